/* libkmbart_hip.so -- C ABI of the MI355X-native KM-BART hot path.
 *
 * The reference (fomalhautb/KM-BART) has no native interface: its hot path is reached through the
 * Python API of src.model / src.training / src.generation.  This header is
 * the boundary a maintainer binds instead (ctypes stub in INTEGRATION.md).  Every entry point
 * cites the reference code whose arithmetic it replaces (paths into the reference checkout).
 *
 * Conventions: plain pointers and sizes only; all data pointers are DEVICE pointers unless the
 * name ends in _host; `stream` is a hipStream_t passed as void*; every function returns 0 on
 * success, non-zero on failure with the message available from kmb_last_error().  Nothing here
 * allocates device memory: the host binds arenas / workspace it owns (torch tensors in the
 * Python host code).  A handle is not thread-safe (one host thread per process per GPU, as
 * the reference's mp.spawn layout, vcg_train.py:350-355).
 */
#ifndef KMBART_H
#define KMBART_H
#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef uint16_t kmb_bf16;            /* raw bfloat16 bits */
typedef struct kmb_handle kmb_handle;

/* src/model/config.py:4-92 + config/vcg_base.json */
typedef struct kmb_config {
  int32_t vocab_size, d_model;
  int32_t encoder_layers, decoder_layers;
  int32_t encoder_attention_heads, decoder_attention_heads;
  int32_t encoder_ffn_dim, decoder_ffn_dim;
  int32_t max_position_embeddings, extra_pos_embeddings;
  int32_t image_feature_size;
  int32_t pad_token_id, bos_token_id, eos_token_id, img_feat_id, cls_token_id;
  int32_t scale_embedding;
  float dropout, attention_dropout, activation_dropout;
  float layer_norm_eps;
  /* pre-training heads (src/model/model.py:133-158); 0 = head absent (MultiModalBartForConditionalGeneration) */
  int32_t num_labels, num_attributes, num_relations;
} kmb_config;

/* one training / scoring batch; layout = what the reference Collator emits
 * (src/data/collation.py:68-213), region features packed row-wise with CSR offsets */
typedef struct kmb_batch {
  int32_t B, S, T;                     /* batch, encoder length, decoder length */
  const int64_t* input_ids;            /* [B,S] */
  const int64_t* attention_mask;       /* [B,S] 1 = keep, or NULL (all ones) */
  const float* image_features;         /* [Ntot, image_feature_size] fp32, rows of sample i at feat_offsets[i] */
  const int32_t* feat_offsets;         /* [B+1] device */
  int32_t n_features;                  /* Ntot (host copy of feat_offsets[B]) */
  const int64_t* decoder_input_ids;    /* [B,T] */
  const int64_t* decoder_attention_mask; /* [B,T] or NULL */
  const int64_t* labels;               /* [B,T], -100 = ignore, or NULL */
} kmb_batch;

/* ---- GEMM with fused epilogue (csrc/gemm.hip) --------------------------------------------- */
typedef struct KmbGemm {
  const kmb_bf16* A; const kmb_bf16* B;
  int32_t lda, ldb;
  int32_t a_kc, b_kc;
  int32_t M, N, K;
  const float* bias;
  float col_scale; int32_t col_scale_n;
  int32_t act;                    /* 0 none, 1 GeLU (erf form), 2 multiply by aux (the stored GeLU'), 3 tanh, 4 multiply by 1 - aux^2,
                                   * 5 exp(v - row_shift[row]) with per-row sums (the tied head's cross-entropy: fields at the end).
                                   * act 1 with drop_thr16 != 0 (activation dropout): the output is keep ? GeLU(v) * drop_scale : 0 and
                                   * preact receives keep ? GeLU'(v) * drop_scale : 0 -- the derivative of what was stored, so an act 2
                                   * launch on it needs no mask.  (Until activation dropout went in, this combination stored the
                                   * UNDROPPED derivative beside a dropped output; nothing in the engine, the tools or the tests
                                   * launched it -- searched: every act 1 launch ran with drop_thr16 = 0, and those return the bits
                                   * they always did.)  Launch variants 8, 14 and 15 do not carry the class and hand it on to 7. */
  kmb_bf16* preact; int32_t ld_preact;   /* act 1, optional: receives GeLU'(pre-activation) -- what the backward pass needs */
  const kmb_bf16* aux; int32_t ld_aux;   /* act 2: the tensor act 1 stored; act 4: tanh output */
  uint32_t drop_thr16; uint32_t drop_seed; float drop_scale;
  const kmb_bf16* residual; int32_t ld_res;
  kmb_bf16* out_bf16; int32_t ld_out_bf16;
  float* out_f32; int32_t ld_out_f32; float beta;
  int32_t split_k; float* slab;   /* split_k > 1: slice s writes raw fp32 accumulators to slab[s][M][N]; no epilogue */
  float* colsum;                  /* optional [ceil(M/64)][N]: per-64-row-block column sums of the stored values */
  int32_t tile_order;             /* set by the launcher (results never depend on it): bit 0 = contiguous tile range per
                                   * XCD; bit 1 = L2 prefetch of the activation panel (persistent kernels); bit 2 = split-K
                                   * (tile, slice) pairs enumerated slice-major: an XCD works on one or two K slices */
  /* act 5 (reference src/model/model.py:397-402 without a pass over the logits): the output is exp(v - row_shift[row]);
   * row_sums[row * row_sums_ld + col / 64] receives, for every 64-column block, the fp32 sum of the row's values in it (a
   * wider wave block puts its whole sum into its first slot and zeros into the others: every slot is written exactly
   * once), pick_out[row] the value v - row_shift[row] at column pick_col[row] (rows whose pick_col is outside [0, N)
   * are not written).  Persistent 256- / 128-column variants only, M and N multiples of 256, bias required. */
  const float* row_shift; float* row_sums; int32_t row_sums_ld; const int64_t* pick_col; float* pick_out;
} KmbGemm;

/* ---- fused attention (csrc/attention.hip) -------------------------------------------------- */
typedef struct KmbAttn {
  const kmb_bf16* Q; const kmb_bf16* K; const kmb_bf16* V;
  int32_t ldq, ldk, ldv;
  int32_t B, H, Tq, Tk;
  const int64_t* key_mask;
  int32_t causal;
  kmb_bf16* O; int32_t ldo;
  float* lse;
  const kmb_bf16* dO; int32_t lddo;
  kmb_bf16* dQ; kmb_bf16* dK; kmb_bf16* dV; int32_t lddq, lddk, lddv;   /* backward: dO, dQ, dK, dV 16-byte aligned, strides multiples of 8 */
  float dq_scale;
  /* optional bias-gradient partials (backward): per-batch-item column sums of dQ (scaled by dq_scale) / dK / dV, fp32, taken from the
   * accumulators before the bf16 rounding; head h of batch item b goes to columns 64 h .. 64 h + 63 of row b, row stride ld_colsum.
   * All three pointers or none (a partial set is refused), and ld_colsum >= 64 H when they are given; the three may share one
   * buffer (training: parts, parts + d, parts + 2 d with ld_colsum = 3 d).  Columns that no head owns are not written. */
  float* dq_colsum; float* dk_colsum; float* dv_colsum; int32_t ld_colsum;
  /* attention dropout (training kernels only; all zero = none): probability element (b, h, q, k) is kept when
   * kmb_op_dropout_mask(drop_seed, thr16 / 65536, B * H * Tq, Tk) keeps element (row (b * H + h) * Tq + q, column k); kept ones are multiplied by
   * drop_scale = 1 / (1 - thr16 / 65536) on their way into P V.  lse stays the undropped softmax's.  Backward must be given the forward's values. */
  uint32_t drop_thr16, drop_seed; float drop_scale;
} KmbAttn;

typedef struct KmbAttnDecode {
  const kmb_bf16* Q; int32_t ldq;
  const kmb_bf16* Kc; const kmb_bf16* Vc;
  int32_t Tmax; int32_t ldc;      /* cache element (row,t,h,e) at X[(row*Tmax + t)*ldc + h*64 + e] */
  const int32_t* kv_row;
  const int64_t* key_mask; int32_t mask_ld;
  const int32_t* mask_row;
  int32_t R, H, Tk;
  kmb_bf16* O; int32_t ldo;
  /* self-attention of a decode step: key / value row Tk-1 is NOT in the cache yet -- it is read from new_k / new_v
   * (row r at new_k + r*ld_new + h*64) and written into caches Kw / Vw at position Tk-1 by the same launch (NULL: plain
   * attention over the cache) */
  const kmb_bf16* new_k; const kmb_bf16* new_v; int32_t ld_new;
  kmb_bf16* Kw; kmb_bf16* Vw;
  /* optional history index of the self-attention cache ([R, Tmax] int32; NULL: a row's history lives in its own cache row): position
   * t < Tk-1 of row r is read from cache row hist[r*Tmax + t]; the launch records hist[r*Tmax + Tk-1] = r for the row it appends.  A beam
   * reorder then permutes these small rows instead of copying the caches (src/model/mixins.py:419-434 _reorder_cache). */
  int32_t* hist;
  /* kmb_op_attn_decode refuses (before any GPU call): Tk < 1 or Tk > Tmax; Tk > 4096 (16 Tk bytes of LDS per workgroup, 64 KB); a missing
   * Q / Kc / Vc / O; new_k, new_v, Kw, Vw not all or none; Q, Kc, Vc, new_k, new_v not 16-byte aligned; ldq, ldc, ld_new not multiples
   * of 8; key_mask with mask_ld < Tk.  R * H <= 0 is nothing to do.  A row whose keys are all masked gets zeros. */
} KmbAttnDecode;

/* One fused block of a KV-cached decode step (csrc/decode.hip): [LayerNorm ->] projection of R rows [-> attention].
 * Replaces the GEMM + attention + LayerNorm launches of one sub-layer of the reference's DecoderLayer under use_cache
 * (transformers 3.0.2 modeling_bart.py:386-466, reached from src/model/mixins.py:386-434).
 *   kind 0: out[R, N] = act(LN?(in) W^T + bias) + residual                         (N % 64 == 0)
 *   kind 1: self-attention of head h = 0..H-1: W = [q | k | v] rows (N = 3*H*64); the new key / value row is written to
 *           the cache at position Tk-1 and attended to together with cache rows 0 .. Tk-2; out[R, H*64]
 *   kind 2: cross-attention: W = q rows (N = H*64); keys / values Kc / Vc of batch item kv_row[row], masked by key_mask
 * K % 768 == 0, K <= 3072 (kinds 1, 2: K = 768).  gamma != NULL: `in` holds pre-LayerNorm sums and the LayerNorm is
 * applied on the way in; ln_out (optional, row stride K) receives the normalised rows once. */
typedef struct KmbDecodeBlock {
  int32_t kind;
  const kmb_bf16* in; int32_t ld_in;
  const float* gamma; const float* beta; float eps;
  kmb_bf16* ln_out;
  const kmb_bf16* W; const float* bias;     /* W: the [N, K] weight in fragment order (kmb_op_decode_pack), bias [N] */
  int32_t R, K, N;
  int32_t act;                              /* kind 0: 1 = GeLU */
  const kmb_bf16* residual; int32_t ld_res; /* kind 0 */
  kmb_bf16* out; int32_t ld_out;
  int32_t H; float q_scale;                 /* kinds 1, 2: (q + bias) * q_scale */
  kmb_bf16* Kc; kmb_bf16* Vc;               /* cache element (row,t,h,e) at X[(row*Tmax + t)*ldc + h*64 + e] */
  int32_t Tmax, ldc, Tk;
  const int32_t* kv_row;                    /* kind 2: cache row (batch item) of every row */
  const int64_t* key_mask; int32_t mask_ld; /* kind 2: key t of cache row c is masked when key_mask[c*mask_ld + t] == 0 */
  int32_t* hist;                            /* kind 1, optional: history index of the cache (see KmbAttnDecode.hist) */
  int32_t kv_group;                         /* kind 2, optional: a promise that kv_row[r] == r / kv_group (beam rows of a
                                             * batch item are consecutive): lets a workgroup stage each item's keys /
                                             * values once for all of its rows.  0: no promise. */
  /* appended (a zeroed record is a bf16 block, as before): the format of W */
  int32_t w_format;                         /* KMB_WFMT_BF16: W as above.  KMB_WFMT_FP8_E4M3: W holds one OCP e4m3 code per element
                                             * (N * K bytes, kmb_op_decode_pack_fp8's order) and row n of the weight is code * 2^w_exp[n];
                                             * the block returns, bit for bit, what the bf16 block returns on those dequantised weights */
  const int8_t* w_exp;                      /* [N] row exponents (4-byte aligned), required by KMB_WFMT_FP8_E4M3 */
} KmbDecodeBlock;
#define KMB_WFMT_BF16 0
#define KMB_WFMT_FP8_E4M3 1

typedef struct KmbDrop { uint32_t thr16; uint32_t seed; float scale; } KmbDrop;
typedef struct KmbAdamW { double lr, beta1, beta2, eps, weight_decay; int32_t step; int32_t correct_bias; float grad_scale; } KmbAdamW;
/* The device record of a clipped / guarded optimizer step (kmb_clip_finish writes it, kmb_adamw_step_dev reads it):
 * norm = the global L2 norm of the gradients before clipping, gradient scaling included; coef = min(1, max_norm / (norm + 1e-6));
 * step_size = lr * sqrt(1 - beta2^steps) / (1 - beta1^steps); applied = 1 if this step updates; steps / skipped = applied and
 * skipped steps so far.  The bias-correction step count of such a step is `steps`, NOT KmbAdamW.step. */
typedef struct KmbStepState { float norm, coef, step_size; int32_t applied, steps, skipped; } KmbStepState;

const char* kmb_last_error(void);
int kmb_version(void);

/* ================= model handle ================= */
/* MultiModalBartForConditionalGeneration(config): src/model/model.py:317-323 */
int kmb_create(const kmb_config* cfg, kmb_handle** out);
void kmb_destroy(kmb_handle* h);

/* parameter census (state-dict names are the reference's: HF BART keys +
 * model.encoder.embed_images.linear.{weight,bias}); offsets are in ELEMENTS into the flat arenas */
int kmb_param_count(const kmb_handle* h);
int kmb_param_info(const kmb_handle* h, int idx, const char** name, int64_t* offset, int32_t* rows, int32_t* cols);
int64_t kmb_arena_elems(const kmb_handle* h);        /* fp32 arenas: params / grads / exp_avg / exp_avg_sq */
int64_t kmb_bf16_arena_elems(const kmb_handle* h);   /* bf16 mirror (+ padded tied matrix + padded image weight) */
int kmb_bind_arenas(kmb_handle* h, float* params, float* grads, float* exp_avg, float* exp_avg_sq,
                    kmb_bf16* params_bf16, float* final_logits_bias);
int64_t kmb_workspace_bytes(const kmb_handle* h, int B, int S, int T, int n_features);
/* ... for a forward with kmb_forward_opts.targets_per_input = G: B inputs of S tokens, B * G targets of T tokens (the encoder side's buffers
 * have B * S rows, the decoder side's B * G * T).  G <= 1: exactly kmb_workspace_bytes. */
int64_t kmb_workspace_bytes_grouped(const kmb_handle* h, int B, int S, int T, int n_features, int targets_per_input);
int kmb_bind_workspace(kmb_handle* h, void* ws, int64_t bytes);
/* refresh the bf16 mirror from the fp32 master parameters (after init / load_state_dict) */
int kmb_sync_params(kmb_handle* h, void* stream);
int kmb_set_seed(kmb_handle* h, uint64_t seed);
/* Attention dropout (the reference's config.attention_dropout: F.dropout on the softmax weights of every attention block).  A run-time
 * setting of the handle -- kmb_create refuses a non-zero kmb_config.attention_dropout -- that takes effect from the next forward; p in [0, 1).
 * Only training-mode forwards (train = 1) and their backward draw masks: eval forwards, kmb_score, generation and the fp32 validation mode
 * run without.  kmb_attention_dropout_site reports what the LAST training forward used at a site (kind 0 encoder self-attention, 1 decoder
 * self-attention, 2 decoder cross-attention; zeros when it ran without): probability (b, h, q, k) was kept where
 * kmb_op_dropout_mask(seed, thr16 / 65536, B * H * Tq, Tk) keeps element ((b * H + h) * Tq + q, k).  With targets_per_input = G > 1
 * (kmb_forward_opts) the decoder self-attention site has B * G items of T x T, and the cross-attention site has B items of Tq = G * T queries
 * against Tk = S keys: its mask is kmb_op_dropout_mask(seed, thr16 / 65536, B * H * G * T, S), query q = g * T + t of input b. */
int kmb_set_attention_dropout(kmb_handle* h, float p);
int kmb_attention_dropout_site(kmb_handle* h, int kind, int layer, uint32_t* thr16, uint32_t* seed);
/* Activation dropout (the reference's config.activation_dropout: F.dropout on gelu(fc1(x)) of every FFN block).  A run-time setting of the
 * handle, exactly like attention dropout -- kmb_create refuses a non-zero kmb_config.activation_dropout -- that takes effect from the next
 * forward; p in [0, 1).  Only training-mode forwards draw masks: eval forwards, kmb_score, generation and the fp32 validation mode run
 * without.  The fc1 GEMM folds the mask into its GeLU output and into the stored GeLU' (KmbGemm.act), so backward neither stores nor redraws
 * it.  kmb_activation_dropout_site reports what the LAST training forward used at a site (kind 0 encoder FFN, 1 decoder FFN; zeros when it
 * ran without): element (row, col) of the [rows, F] hidden activations (rows = B * S for the encoder, B * T for the decoder, F the FFN
 * width) was kept where kmb_op_dropout_mask(seed, thr16 / 65536, rows, F) keeps it. */
int kmb_set_activation_dropout(kmb_handle* h, float p);
int kmb_activation_dropout_site(kmb_handle* h, int kind, int layer, uint32_t* thr16, uint32_t* seed);
/* Classification-head dropout (the reference's config.classif_dropout: HF 3.0.2 BartClassificationHead drops its input and its tanh output,
 * two independent F.dropout calls per head, src/model/model.py:133-158).  A run-time setting of the handle like the two above -- kmb_config
 * keeps its layout and kmb_create does not learn it -- that takes effect from the next training-mode forward; p in [0, 1).  Only
 * kmb_forward_pretrain* with train = 1 draws masks: eval forwards, kmb_score and generation run without, and a model without heads has
 * nothing to drop.  kmb_classif_dropout_site reports what the LAST training forward used at a site (head 0 masked-region, 1 attribute,
 * 2 relation; which 0 the head's input, 1 its hidden tanh output; zeros when that forward ran without, when the head had no rows, or when
 * the model has no such head): element (row, col) of the head's gathered input [n, d_in] (d_in = d_model, 2 d_model = object | subject for
 * the relation head) or of its hidden activations [n, d_model] was kept where kmb_op_dropout_mask(seed, thr16 / 65536, n, d_in or d_model)
 * keeps it; kept elements are multiplied by 1 / (1 - thr16 / 65536). */
int kmb_set_classif_dropout(kmb_handle* h, float p);
int kmb_classif_dropout_site(kmb_handle* h, int head, int which, uint32_t* thr16, uint32_t* seed);
/* Label smoothing of the LM cross-entropy (fairseq's label_smoothed_cross_entropy / torch's CrossEntropyLoss(label_smoothing = eps)):
 *   loss = mean over rows with a label in [0, V) of  lse(v_r) - (1 - eps) v_r[label_r] - eps mean_{j < V} v_rj
 * and its gradient (softmax - (1 - eps) onehot - eps / V) / count.  A run-time setting of the handle like the dropout settings above
 * (kmb_config keeps its layout); 0 <= eps < 1, anything else (NaN included) is refused with a message.  It applies to every forward
 * with labels from the next one on -- kmb_forward*, kmb_forward_pretrain* (the LM term), train and eval alike, whichever head form runs.
 * kmb_score and generation are untouched.  With the fused tied head the smoothing terms never touch the [rows, V] matrix: with
 * wsum = sum_{j < V} E_j and bsum = sum_{j < V} b_j the row mean is (h_r . wsum + bsum) / V, the label's entry of the stored matrix becomes
 * bf16(1 - (1 - eps) S_r), the uniform part is dH_r -= beta_r wsum and dE_j -= u for every j < V with beta_r = eps lm_factor / (count V) and
 * u = sum_r beta_r h_r.  eps = 0 (the default) runs exactly the launches it ran without the setting.
 * kmb_last_head_form: which head the last forward with labels took -- 0 fp32 logits + cross-entropy, 1 bf16 logits turned into their
 * gradient in place, 2 the fused head (no logits pass); -1 before the first such forward. */
int kmb_set_label_smoothing(kmb_handle* h, float eps);
int kmb_last_head_form(const kmb_handle* h);
int kmb_abi_sizeof_attn(void);   /* sizeof(KmbAttn) as the library was compiled: a binding checks its own layout against it */

/* gradient buckets for data-parallel overlap (DDP reducer, vcg_train.py:98): bucket i is complete
 * on the compute stream once kmb_backward has passed its event */
int kmb_bucket_count(const kmb_handle* h);
int kmb_bucket_range(const kmb_handle* h, int i, int64_t* offset, int64_t* count);
int kmb_stream_wait_bucket(kmb_handle* h, int i, void* stream);

/* ================= training step ================= */
/* MultiModalBartForConditionalGeneration.forward, src/model/model.py:325-405
 * (encoder src/model/modules.py:104-165, ImageEmbedding :24-41, _embed_multi_modal :89-102).
 *   train       : dropout active (model.train())
 *   need_grad   : also produce what kmb_backward needs (and the tied-head gradients)
 *   loss_out    : device float[1] (mean CE over labels != -100), may be NULL when labels == NULL
 *   logits_out  : device float [B*T, kmb_logits_ld()] or NULL; columns >= vocab_size are padding
 *   enc_out     : device bf16 [B*S, d_model] or NULL (encoder_last_hidden_state copy) */
int kmb_logits_ld(const kmb_handle* h);
int kmb_forward(kmb_handle* h, const kmb_batch* batch, int train, int need_grad, float* loss_out,
                float* logits_out, kmb_bf16* enc_out, void* stream);
/* Scores of a GIVEN target sequence: log p(label_t | image, event, labels_<t) per decoder position and per sample, without
 * materialising the logits (reference scripts/filter_reason.py:24-52 -- forward without labels, log_softmax over outputs[0], the
 * label's entry token by token, the mean over labels >= 0 against --pp_threshold).  An eval-mode forward (no dropout, need_grad = 0)
 * that counts as a forward: it rewrites the workspace and invalidates a pending kmb_backward.  batch->labels is required.
 *   token_logprob [B*T] fp32 : log_softmax(logits)[label]; 0 where the label is -100 or outside [0, vocab_size)
 *   sample_nll    [B]   fp32 : the SUM of -token_logprob over the item's valid rows, in row order (no floating-point atomics)
 *   sample_count  [B]   int32: the number of valid rows (0: the caller's mean / perplexity is 0 / 0 = NaN)
 *   path_out (HOST, may be NULL): 1 = the store-free head ran, 0 = the fallback
 * Store-free head: at least 256 decoder rows, padded vocabulary % 256 == 0, d_model % 64 == 0 and >= 320, bf16 product mode.  The
 * label's logit comes from 2 * d_model values per row; one GEMM over the rows ROUNDED UP to whole 256-row tiles keeps, per row and
 * 64-column block, the block's maximum and sum-exp only -- exact for any finite logits (nothing is shifted by the label's logit, no
 * exponent is clamped), a non-finite logit makes its own row's score non-finite.  The TAIL ROWS [B*T, round_up(B*T, 256)) are whatever
 * the bound workspace holds behind the decoder states (always inside it); rows of a GEMM are independent, their statistics go to rows
 * of their own in the workspace and nothing reads them.  Fallback (anything else, and KMB_SCORE_FALLBACK=1 in the environment, read
 * per call): fp32 logits in row chunks bounded by the workspace's existing head scratch + the row cross-entropy kernel; the fp32
 * validation mode always takes it, through the fp32 head.  Out-of-range labels set bit 1 of the status word (kmb_read_status), as in
 * kmb_forward.  Workspace: kmb_workspace_bytes, unchanged. */
int kmb_score(kmb_handle* h, const kmb_batch* batch, float* token_logprob /* [B*T] */, float* sample_nll /* [B] */,
              int32_t* sample_count /* [B] */, int32_t* path_out /* host, may be NULL */, void* stream);
/* Optional inputs / outputs of the forward that the bare MultiModalBartModel and the `encoder_outputs` keyword need
 * (src/model/model.py:39-103): */
typedef struct kmb_forward_opts {
  const kmb_bf16* encoder_states;   /* [B*S, d_model] or NULL: skip the encoder and use these states (model.py:76-83) */
  kmb_bf16* decoder_states_out;     /* [B*T, d_model] or NULL: copy of the last decoder hidden states (model.py:87-103) */
  int32_t skip_head;                /* 1: stop after the decoder (no logits, no loss): MultiModalBartModel.forward */
  /* Per-row weights of the LM cross-entropy: L = sum_r w_r nll_r / D over the rows with a valid label, nll_r with
   * the label-smoothing term when that is on; the logits-gradient row is w_r lm_factor / D (softmax - target).  Negative and zero weights
   * are legal; a row whose label is -100 or out of range contributes exactly zero loss and an exactly zero gradient row whatever its
   * weight holds (NaN included: it is not read).  Honoured by all three head forms and by the fp32 validation mode's loss; only the LM
   * term is weighted (kmb_forward_pretrain_ex: lm_factor multiplies the weighted term, the other heads are untouched).  row_weights
   * without labels is refused.  NULL and loss_reduction 0 run exactly the launches kmb_forward runs. */
  const float* row_weights;         /* [B*T] fp32 on the device, indexed like labels, or NULL */
  int32_t loss_reduction;           /* 0 mean: D = the number of valid labels (NaN without one); 1 sum: D = 1 (exactly 0 without one) */
  /* Several targets per input, the encoder run once.  0 and 1: one target per input, exactly the launches that ran
   * without the field.  It sits in what was the struct's tail padding, so sizeof -- and kmb_abi_sizeof_forward_opts -- is unchanged and cannot
   * tell a caller compiled against the older header from a new one: ZERO THE WHOLE RECORD (memset(&opts, 0, sizeof opts), `kmb_forward_opts o{}`,
   * `= {0}`) before filling it, as every caller in this repository does.  A record whose fields were assigned one by one on an uninitialised
   * stack slot now passes whatever the padding held as G; such a value is refused when negative or when G * T > 384, not otherwise.  G > 1: batch->B, S, input_ids, attention_mask and
   * the features describe B inputs as before; decoder_input_ids, decoder_attention_mask and labels are [B * G, T] with decoder row i belonging to
   * input i / G (the row order of generate(num_return_sequences = G)); row_weights [B * G * T]; logits_out / kmb_last_logits
   * [B * G * T, kmb_logits_ld()]; decoder_states_out [B * G * T, d_model]; enc_out and encoder_states stay [B * S, d_model] (kmb_encoder_states_grad
   * likewise: the gradient summed over an input's G targets).  The decoder's self-attention runs B * G causal items of T x T; cross-attention runs
   * B items of Tq = G * T queries against the input's S keys, not causal -- at S <= 64 the query-streaming kernels (kmb_debug_attn_route) -- and
   * its key | value gradient arrives summed over the G targets.  Workspace: kmb_workspace_bytes_grouped.  Refused before any launch: G < 0,
   * G * T > 384 (the attention backward's query limit), G > 1 in kmb_forward_pretrain*.  kmb_score always scores one target per input, and
   * kmb_attention_probs is refused after a grouped forward. */
  int32_t targets_per_input;
} kmb_forward_opts;
int kmb_abi_sizeof_forward_opts(void);   /* sizeof(kmb_forward_opts) as the library was compiled (cf. kmb_abi_sizeof_attn) */
/* kmb_forward with those options.  With encoder_states AND need_grad the following kmb_backward stops at the given states:
 * the encoder's parameter gradients are zero, dL / d states comes from kmb_encoder_states_grad (the reference's
 * `forward(encoder_outputs=...)` with a tensor that requires grad, src/model/model.py:76-83).  In the fp32 validation mode the
 * kmb_bf16 pointers of kmb_forward / kmb_forward_ex carry floats (kmb_act_bytes() == 4). */
int kmb_forward_ex(kmb_handle* h, const kmb_batch* batch, const kmb_forward_opts* opts, int train, int need_grad,
                   float* loss_out, float* logits_out, kmb_bf16* enc_out, void* stream);
/* logits [B*T, kmb_logits_ld()] of the decoder states the LAST forward left in the workspace: `outputs[1]` of a training
 * forward (src/model/model.py:397-405) as one extra head GEMM instead of 1.6 GB written every step */
int kmb_last_logits(kmb_handle* h, float* logits_out, void* stream);
/* `output_hidden_states` / `output_attentions` of the forward still in the workspace (reference src/model/modules.py:143-165,
 * transformers 3.0.2 BartDecoder): hidden state `index` of the encoder (which = 0: 0 .. encoder_layers, 0 = the embedding
 * output, l + 1 = the output of layer l) or of the decoder (which = 1: 0 .. decoder_layers) as [rows, d_model] activations,
 * and the self-attention probabilities of layer `layer` as fp32 [B, H, T, T], recomputed from the saved q | k and the rows'
 * log-sum-exp (the fused attention kernels never store them).  bf16 product mode only. */
int kmb_hidden_state(kmb_handle* h, int which, int index, kmb_bf16* out, void* stream);
int kmb_attention_probs(kmb_handle* h, int which, int layer, float* out, void* stream);
/* dL / d(encoder output) of the last kmb_backward as bf16 [B*S, d_model] (what autograd hands to `encoder_outputs[0].grad`) */
int kmb_encoder_states_grad(kmb_handle* h, kmb_bf16* out, void* stream);
/* fp32 VALIDATION mode (1) / bf16 product mode (0, default).  Mode 1 keeps every activation in float and runs the
 * eval-mode forward on exact-fp32 kernels (csrc/fp32_validate.hip) against the fp32 master weights: parity evidence for
 * north_star's "logits within 1e-3 of the fp32 reference path", never the measured path.  Training, backward and
 * generation are refused in mode 1.  Rebind the workspace after switching (kmb_workspace_bytes doubles). */
int kmb_set_precision(kmb_handle* h, int fp32);
int kmb_act_bytes(const kmb_handle* h);
/* loss.backward() (src/training.py:138,142); loss_scale multiplies every gradient */
int kmb_backward(kmb_handle* h, float loss_scale, void* stream);
/* the same with the scale as a DEVICE scalar: autograd hands `loss.backward()` its upstream gradient (ones, or the
 * GradScaler's scale, src/training.py:137-142) as a device tensor; reading it on the device keeps the API path free of a
 * host synchronisation.  A scale of exactly 1 costs three early-exit launches. */
int kmb_backward_dev(kmb_handle* h, const float* loss_scale_dev, void* stream);
/* transformers.AdamW.step (vcg_train.py:100, src/training.py:139,143) over [offset, offset+count) */
int kmb_adamw_step(kmb_handle* h, const KmbAdamW* hp, int64_t offset, int64_t count, void* stream);
/* ---- clipped / guarded step: global gradient-norm clipping (torch.nn.utils.clip_grad_norm_, L2) and the skip of a step whose
 * gradients are not finite (what GradScaler.step does), decided ON THE DEVICE before any parameter moves.
 *   kmb_grad_sumsq (one call per contiguous piece, each into its own block of partial slots)  ->  kmb_clip_finish (once)  ->
 *   kmb_adamw_step_dev (per piece)
 * The step-state buffer is the caller's: a KmbStepState record followed (at byte 64) by double partial sums, kmb_step_state_bytes in all.
 * It must NOT live in the workspace (the bias-correction step count has to survive whatever rewrites that); kmb_bind_step_state
 * zeroes it (synchronously).  Nothing here synchronises the host except the bind. */
int64_t kmb_step_state_bytes(const kmb_handle* h);
int kmb_bind_step_state(kmb_handle* h, void* buf, int64_t bytes);
/* partial sums of (G[i] * grad_scale)^2 over [offset, offset + count) (offset a multiple of 4) into slots [slot0, slot0 +
 * kmb_op_grad_sumsq_slots(count)); the sums are doubles, one per workgroup, no atomics: the same pieces give the same bits */
int kmb_grad_sumsq(kmb_handle* h, int64_t offset, int64_t count, float grad_scale, int32_t slot0, void* stream);
/* sums slots [0, nslots) and writes the record; max_norm <= 0: no clipping; hp: lr, betas and correct_bias are read (hp->step is not) */
int kmb_clip_finish(kmb_handle* h, const KmbAdamW* hp, float max_norm, int32_t skip_nonfinite, int32_t nslots, void* stream);
/* kmb_adamw_step under the record: nothing moves when applied == 0; otherwise gradients are scaled by hp->grad_scale * coef and the
 * record's step_size is used.  Same range rules and the same image-weight re-pad as kmb_adamw_step. */
int kmb_adamw_step_dev(kmb_handle* h, const KmbAdamW* hp, int64_t offset, int64_t count, void* stream);
/* asynchronous copy of the record to host_record (page-locked memory); the caller synchronises the stream before reading */
int kmb_step_state_read(kmb_handle* h, KmbStepState* host_record, void* stream);
/* sets the record's applied-step count (loading a checkpoint), in stream order */
int kmb_step_state_set_steps(kmb_handle* h, int32_t steps, void* stream);
/* ---- gradient accumulation over micro-batches.  Every gradient writer of a forward + backward overwrites; with accumulation on they
 * write this micro-batch's gradient into a second fp32 arena of the same layout, the STAGE, and kmb_backward folds each bucket of it into
 * the gradient arena right before it records that bucket's completion event: G = stage for the first backward after kmb_zero_grad, G +=
 * stage for later ones.  A bucket's event (kmb_stream_wait_bucket) then means "the ACCUMULATED gradient of this bucket is complete", and
 * every reader (kmb_adamw_step*, kmb_grad_sumsq, kmb_allreduce_grads, the caller's views of the arena) sees the running total.
 * The stage is the caller's buffer of at least kmb_arena_elems floats, 256-byte aligned, zero-filled (the alignment gaps between
 * parameters are never written and are folded like everything else), outside the workspace: that is rewritten and re-laid out per
 * micro-batch.  A bound stage must outlive accumulation (switch it off before freeing the buffer). */
int kmb_bind_grad_stage(kmb_handle* h, float* stage, int64_t floats);
/* on != 0: gradient writers target the stage and kmb_backward folds; 0 (default): the writers target the gradient arena, as without this
 * call.  Fails between a need_grad forward and its backward (that forward's gradients already went to one of the two), and when switched
 * on without a bound stage.  Switching on starts as if kmb_zero_grad had been called. */
int kmb_set_grad_accumulation(kmb_handle* h, int on);
/* the next kmb_backward's folds overwrite the gradient arena instead of adding to it (they never read it).  A host flag, no launch; read
 * when backward runs (forward -> kmb_zero_grad -> backward is the reference's order, src/training.py:136) and cleared by it.  No effect
 * while accumulation is off. */
int kmb_zero_grad(kmb_handle* h);
/* status word written by device-side input validation (bit 0: #<img_feat> ids != #region rows) */
int kmb_read_status(kmb_handle* h, int32_t* status_host, void* stream);
/* The same without the synchronisation: the status word is copied to `status_host` (page-locked memory) in stream order; the
 * caller reads it after a later synchronisation of that stream (generation: at the end of generate(), so that the decode
 * steps are enqueued while the encoder still runs). */
int kmb_read_status_async(kmb_handle* h, int32_t* status_host, void* stream);

/* ---- multi-task pre-training (MultiModalBartForPreTraining.forward, src/model/model.py:162-309) ----
 * rows index the flattened decoder positions [B*T]; every pointer is a device pointer; n_* may be 0 */
typedef struct kmb_pretrain {
  int32_t n_mrm; const int32_t* mrm_rows; const float* mrm_targets;     /* soft labels [n_mrm, num_labels] (model.py:248-257) */
  int32_t n_attr; const int32_t* attr_rows; const int64_t* attr_labels; /* (model.py:259-268) */
  int32_t n_rel; const int32_t* rel_obj_rows; const int32_t* rel_subj_rows; const int64_t* rel_labels; /* (:270-289) */
  float lm_factor, mrm_factor, attr_factor, rel_factor;                 /* config.*_loss_factor (:304-307) */
  float* losses_out;                                                    /* device float[5]: loss, lm, mrm, attribute, relation */
} kmb_pretrain;
/* room for up to n gathered head rows in the workspace (call before kmb_workspace_bytes) */
int kmb_reserve_head_rows(kmb_handle* h, int n);
/* kmb_forward plus the three classification heads; `labels` must already carry -100 at <cls> positions (:297-298) */
int kmb_forward_pretrain(kmb_handle* h, const kmb_batch* batch, const kmb_pretrain* extra, int train, int need_grad,
                         float* logits_out, kmb_bf16* enc_out, void* stream);
/* ... with a kmb_forward_opts record -- encoder_states: the reference passes `encoder_outputs` through to self.model,
 * src/model/model.py:225-242; decoder_states_out; skip_head is refused */
int kmb_forward_pretrain_ex(kmb_handle* h, const kmb_batch* batch, const kmb_pretrain* extra, const kmb_forward_opts* opts,
                            int train, int need_grad, float* logits_out, kmb_bf16* enc_out, void* stream);

/* ================= generation ================= */
/* encoder once (src/model/mixins.py:281-283) + cross-attention K/V of every decoder layer.  Asynchronous: everything is
   enqueued on `stream` and the call returns without synchronising (the batch's device buffers must stay valid until the
   generation's last kmb_gen_step has run). */
int kmb_gen_begin(kmb_handle* h, const kmb_batch* batch, int num_beams, int max_length, void* stream);
/* encoder output [B*S, d_model] (bf16) of the kmb_gen_begin still active: the `encoder_outputs` element of the cached
 * forward's return tuple (src/model/model.py:384-397 returns decoder_outputs + encoder_outputs) */
int kmb_gen_encoder_states(kmb_handle* h, kmb_bf16* enc_out, void* stream);
/* one cached decoder step (src/model/mixins.py:386-398 -> model.py:384-397): tokens [B*num_beams]
 * at position `step` (0-based), logits_out fp32 [B*num_beams, kmb_logits_ld()].  A non-NULL `tokens` is always embedded.
 * tokens = NULL: the step runs on the tokens the preceding kmb_gen_beam_step(reorder_step = step - 1) chose and already
 * embedded (no embedding launch); fails when no such embedding is pending for `step` (kmb_gen_embedded_step). */
int kmb_gen_step(kmb_handle* h, const int64_t* tokens, int step, float* logits_out, void* stream);
/* the step whose tokens the last kmb_gen_beam_step (or kmb_gen_beam_sample_step, kmb_gen_greedy_step,
 * kmb_gen_sample_step) embedded for a kmb_gen_step(tokens = NULL), or -1: none pending (any
 * kmb_gen_step or kmb_gen_beam_step since, or that beam step did not embed -- no reorder, no next step inside max_length, or the
 * decoder states kmb_gen_last_hidden returns still lived where the embedding goes).  Host state only: no stream work. */
int kmb_gen_embedded_step(const kmb_handle* h);
/* the number of 256-column blocks of (maximum, sum-exp) statistics the last kmb_gen_step's vocabulary projection left for `logits` (the
 * logits_out it was given), or 0: none -- another GEMM kernel ran (not 257 .. 320 beam rows), KMB_GEN_HEAD_STATS=0, no projection, or other
 * logits.  While it is > 0, kmb_gen_beam_step on those logits without a forced token selects from the statistics in one launch.  Host state
 * only: no stream work. */
int kmb_gen_stats_blocks(const kmb_handle* h, const float* logits);
/* _reorder_cache (src/model/mixins.py:419-434): self-attention caches follow beam_idx [B*num_beams] -- through their history
 * index (KmbAttnDecode.hist), which one launch permutes; the caches themselves are never copied */
int kmb_gen_reorder(kmb_handle* h, const int32_t* beam_idx, int step, void* stream);
/* The final decoder states of the last kmb_gen_step as bf16 [rows, d_model] (the `decoder_outputs[0]` of a cached bare-model
 * forward, reference src/model/model.py:87-103 with use_cache; transformers 3.0.2 BartDecoder returns the one new position). */
int kmb_gen_last_hidden(kmb_handle* h, kmb_bf16* out, void* stream);
/* log_softmax + top-k per row of (logp + add[row]); force_token >= 0 forces that token
 * (adjust_logits_during_generation, src/model/mixins.py:400-417); ban_token >= 0 scores that token -inf AFTER the
 * normalisation (min_length: transformers 3.0.2 postprocess_next_token_scores acts on the log-probabilities) */
int kmb_logsoftmax_topk(const float* logits, int ld, int V, int rows, const float* add, int force_token, int ban_token,
                        int k, float* out_val, int32_t* out_idx, void* stream);
/* the same with a scratch buffer of kmb_logsoftmax_topk_scratch(rows) floats: every row is split over four workgroups and
 * combined by a second launch -- the form the decode loop uses (a few hundred rows); results are identical up to the
 * rounding of the log-sum-exp */
int64_t kmb_logsoftmax_topk_scratch(int rows);
int kmb_logsoftmax_topk_ws(const float* logits, int ld, int V, int rows, const float* add, int force_token, int ban_token,
                           int k, float* out_val, int32_t* out_idx, float* scratch, int64_t scratch_floats, void* stream);
/* one beam-search step's candidate selection (mixins.py beam loop: topk over num_beams * V): per batch item the best k of
 * its beams' top-k lists; out[B][k][2] int32 = {fp32 score bits, beam * V + token} */
int kmb_beam_merge(const float* val, const int32_t* idx, int B, int num_beams, int k, int V, int32_t* out, void* stream);
/* the same, and the beams of the next decode step chosen on the device: in candidate order the first num_beams candidates
 * whose token is not eos_token (-1: none) -> next_scores [B*num_beams] (the `add` of the next kmb_logsoftmax_topk),
 * next_tokens [B*num_beams] (int64, the next kmb_gen_step), next_beam_idx [B*num_beams] (kmb_gen_reorder): the selection
 * of transformers 3.0.2 _generate_beam_search (reached from src/model/mixins.py:336-361) without its host round trip;
 * `out` still carries every candidate for the host's hypothesis bookkeeping. */
int kmb_beam_merge_select(const float* val, const int32_t* idx, int B, int num_beams, int k, int V, int32_t* out,
                          int eos_token, float* next_scores, int64_t* next_tokens, int32_t* next_beam_idx, void* stream);
/* kmb_logsoftmax_topk_ws over the B * num_beams rows + kmb_beam_merge_select in two launches instead of three (one when the
 * token is forced): the per-row top-k lists stay in the workgroup that merges them.  Same outputs as the two calls
 * (src/model/mixins.py:336-361, one beam-search step).  Fails for shapes the fused form does not cover (k > 16,
 * num_beams > 16, num_beams * k > 256): use the two calls. */
int kmb_beam_step(const float* logits, int ld, int V, int B, int num_beams, const float* add, int force_token, int ban_token,
                  int k, int32_t* out, int eos_token, float* next_scores, int64_t* next_tokens, int32_t* next_beam_idx,
                  float* scratch, int64_t scratch_floats, void* stream);
/* The decode loop's form of kmb_beam_step, on the logits the last kmb_gen_step wrote (`logits` / `ld` as passed there; V and B are
 * the handle's): same arguments, outputs and selection.  When that step's vocabulary projection ran the all-rows kernel
 * (257 .. 320 beam rows -- the benchmarked 64 x 5) it also left every row's maximum and sum-exp per 256-column block, and ONE
 * launch takes the row's log-sum-exp from those and reads only the blocks that can hold one of the k best, instead of
 * streaming the logits a second time; the scores then differ from kmb_beam_step's in the last bits (the log-sum-exp is
 * grouped by 197 blocks instead of 4 parts), ties still go to the smaller index.  Any other shape, a forced token, or
 * KMB_GEN_HEAD_STATS=0 in the environment: kmb_beam_step itself.  Reference: one step of transformers 3.0.2
 * _generate_beam_search as reached from src/model/mixins.py:336-361, scores adjusted as in mixins.py:386-417.
 * reorder_step >= 0: the call is also kmb_gen_reorder(h, next_beam_idx, reorder_step, stream) (_reorder_cache,
 * src/model/mixins.py:419-434) -- with the history index by the launch that has just chosen the beams; -1: no reorder.  It
 * then usually also embeds next_tokens for step reorder_step + 1: kmb_gen_embedded_step() tells, and kmb_gen_step(h, NULL,
 * reorder_step + 1, ...) uses them.  The statistics belong to the logits as kmb_gen_step wrote them: a caller that edits
 * those logits (masks, penalties) between the two calls must use kmb_beam_step (+ kmb_gen_reorder) instead. */
int kmb_gen_beam_step(kmb_handle* h, const float* logits, int ld, int num_beams, const float* add, int force_token, int ban_token,
                      int k, int32_t* out, int eos_token, float* next_scores, int64_t* next_tokens, int32_t* next_beam_idx,
                      float* scratch, int64_t scratch_floats, int reorder_step, void* stream);
/* One decode step's sampling tail of generate(do_sample=True, num_beams=1) (transformers 3.0.2 _generate_no_beam_search as
 * reached from the reference's nucleus sampling, src/generation.py:22-32; filter = src/model/model.py top_k_top_p_filtering),
 * ONE launch, no sort; stateless like kmb_beam_step.  Per row r < R of logits [R, ld] (fp32, V real columns):
 * x = logits[r, :V] with x[ban_token] = -inf (ban_token -1: none; the min_length EOS ban), NaN read as -inf; x / temperature
 * (correctly rounded); top_k > 0: remove x < the min(top_k, V)-th largest value (ties with it stay); top_p < 1: over the
 * survivors ranked by (value descending, index ascending), keep a token iff the softmax mass ranked before it is <= top_p
 * (the first always); token = argmax over the kept i of softmax_i / noise[r, i] (lowest index on ties), noise [R, ld_noise]
 * fp32 Exp(1) draws supplied by the caller and read at kept tokens only -- torch.multinomial(p, 1)'s exponential race.
 * unfinished (int64 [R], or NULL): a finished row takes pad_token, then unfinished[r] &= token != eos_token (-1: none).
 * The token goes to next_tokens[r] (int64, the next kmb_gen_step's input) and, when ids != NULL, to ids[r * ld_ids + t];
 * flag (int32, or NULL) is OR-ed with 1 when a row is still unfinished; info_out (fp32 [R, 2], or NULL) receives the number
 * of kept tokens and the smallest kept value.  Deterministic: integer atomics only.  1 <= V <= 65536. */
int kmb_sample_step(const float* logits, int ld, int V, int R, float temperature, int top_k, float top_p, int ban_token,
                    const float* noise, int ld_noise, int64_t* unfinished, int64_t pad_token, int64_t eos_token,
                    int64_t* next_tokens, int64_t* ids, int t, int ld_ids, int32_t* flag, float* info_out, void* stream);
/* kmb_sample_step that also says how likely its token was: the same launch, the same tokens and outputs for the same inputs, and
 * lp = log(m_tok / sum of m_i over the kept i), m_i = exp(x_i - max x) -- the chosen token's log-probability under the distribution
 * it was drawn from, i.e. after the EOS ban, NaN -> -inf, the division by the temperature, top-k and top-p (log_softmax of the
 * filtered logits at the token: the `_scores` of the reference's sample_sentence, src/model/utils.py:30-36).  m is the mass the draw
 * itself uses: 1 at the row maximum even when that is infinite, so lp is finite and <= 0 -- 0 when one token is kept,
 * -log(number kept) for an all -inf or all-NaN row.  (Finite for finite positive noise, which Exp(1) draws are: only an infinite
 * or NaN noise value at the maximum lets a kept token of mass 0 win the race, and its lp is -inf.)
 * logprob_sum (fp32 [R], or NULL): logprob_sum[r] += lp for the rows that were unfinished on entry (every row without
 * `unfinished`) -- the EOS token's own lp included, a finished row adds nothing: sample_sentence's sum_logprobs
 * (src/model/utils.py:52-56).  logprob_out (fp32, or NULL): element r at logprob_out[r * ld_logprob] (ld_logprob >= 1; a column of
 * a [R, max_length] buffer is written in place) receives this step's lp, 0 for a finished row.
 * Deterministic: the kept masses are added in a fixed order, no floating-point atomics.  Bad arguments fail with a message and
 * launch nothing. */
int kmb_sample_scored_step(const float* logits, int ld, int V, int R, float temperature, int top_k, float top_p, int ban_token,
                           const float* noise, int ld_noise, int64_t* unfinished, int64_t pad_token, int64_t eos_token,
                           int64_t* next_tokens, int64_t* ids, int t, int ld_ids, int32_t* flag, float* info_out, float* logprob_sum,
                           float* logprob_out, int ld_logprob, void* stream);
/* The decode loop's form of kmb_sample_scored_step on the logits the last kmb_gen_step wrote (V and R are the handle's; needs
 * kmb_gen_begin with num_beams == 1): same outputs.  embed_step as in kmb_gen_greedy_step: >= 0, the same launch also embeds the
 * chosen tokens for decode step embed_step (kmb_gen_step's own row code, bit-identical rows) into the generation workspace --
 * unless that step lies outside the cache or d_model is not a multiple of 8 or > 1024: kmb_gen_embedded_step() tells, and
 * kmb_gen_step(h, NULL, embed_step, ...) uses the rows.  kmb_gen_last_hidden keeps returning the step's decoder states.
 * embed_step -1: no embedding. */
int kmb_gen_sample_step(kmb_handle* h, const float* logits, int ld, float temperature, int top_k, float top_p, int ban_token,
                        const float* noise, int ld_noise, int64_t* unfinished, int64_t pad_token, int64_t eos_token,
                        int64_t* next_tokens, int64_t* ids, int t, int ld_ids, int32_t* flag, float* info_out, float* logprob_sum,
                        float* logprob_out, int ld_logprob, int embed_step, void* stream);
/* One decode step's greedy tail of generate(num_beams=1, do_sample=False) (transformers 3.0.2 _generate_no_beam_search, the
 * mode the reference runs by default: vcg_generate.py --num_beams 1, the training callback of vcg_train.py:183-194), ONE
 * launch, one pass over the logits; stateless like kmb_sample_step, whose argument conventions it keeps.  Per row r < R of
 * logits [R, ld] (fp32, V real columns; columns >= V are never read): x = logits[r, :V], NaN read as -inf, x[ban_token] = -inf
 * (ban_token -1: none; the min_length EOS ban, applied to the logits before any normalisation as postprocess_next_token_scores
 * does there); token = argmax x, the lowest index on exact ties; lp = x[token] - logsumexp(x); a row with no finite entry
 * gives token 0 and lp = -inf.
 * unfinished (int64 [R], or NULL): a finished row takes pad_token, then unfinished[r] &= token != eos_token (-1: none).
 * The token goes to next_tokens[r] (int64, the next kmb_gen_step's input) and, when ids != NULL, to ids[r * ld_ids + t];
 * flag (int32, or NULL) is OR-ed with 1 when a row is still unfinished.
 * logprob_sum (fp32 [R], or NULL): logprob_sum[r] += lp for the rows that were unfinished on entry (every row without
 * `unfinished`) -- the EOS token's own log-probability included, a finished row adds nothing: the sum_logprobs of the
 * reference's sample_sentence (src/model/utils.py:34-56).  logprob_out (fp32 [R], or NULL) receives this step's lp, 0 for a
 * finished row.  Any V >= 1, ld >= V, R >= 1 (rows that do not start on 16 bytes are read one column per load).
 * Deterministic: a fixed reduction order, no floating-point atomics.  Bad arguments fail with a message and launch nothing. */
int kmb_greedy_step(const float* logits, int ld, int V, int R, int ban_token, int64_t* unfinished, int64_t pad_token, int64_t eos_token,
                    int64_t* next_tokens, int64_t* ids, int t, int ld_ids, int32_t* flag, float* logprob_sum, float* logprob_out,
                    void* stream);
/* The decode loop's form of kmb_greedy_step on the logits the last kmb_gen_step wrote (V and R are the handle's; needs
 * kmb_gen_begin with num_beams == 1): same outputs.  embed_step >= 0: the same launch also embeds the chosen tokens for decode
 * step embed_step (token embedding + position extra_pos_embeddings + embed_step + layernorm_embedding, kmb_gen_step's own row
 * code, bit-identical rows) into the generation workspace -- unless that step lies outside the cache or d_model is not a
 * multiple of 8 or > 1024: kmb_gen_embedded_step() tells, and kmb_gen_step(h, NULL, embed_step, ...) uses the rows.
 * kmb_gen_last_hidden keeps returning the step's decoder states.  embed_step -1: no embedding. */
int kmb_gen_greedy_step(kmb_handle* h, const float* logits, int ld, int ban_token, int64_t* unfinished, int64_t pad_token,
                        int64_t eos_token, int64_t* next_tokens, int64_t* ids, int t, int ld_ids, int32_t* flag, float* logprob_sum,
                        float* logprob_out, int embed_step, void* stream);
/* generate()'s score processors on one decode step's logits, in place, in front of kmb_greedy_step / kmb_sample_step (transformers
 * 3.0.2 postprocess_next_token_scores as _generate_no_beam_search applies it, in its order; the arguments the reference validates in
 * src/model/mixins.py:150-235).  ONE launch, one workgroup per row, no pass over [R, V]; stateless like kmb_greedy_step.  Per row
 * r < R of logits [R, ld] (fp32, V real columns), with the row's tokens so far ids[r * ld_ids + 0 .. t) (int64; t = the column the
 * step behind this call writes; a token outside [0, V) is dropped from the row as if it had not been generated):
 *   repetition_penalty p != 1: every DISTINCT token of the row once, v = logits[r, token] becomes v < 0 ? v * p : v * (1 / p), the
 *     reciprocal rounded to fp32 once (what torch's device kernel computes for tensor / python_scalar);
 *   no_repeat_ngram_size n > 0 with t + 1 >= n: every j <= t - n whose n - 1 tokens equal the row's last n - 1 sets
 *     logits[r, row[j + n - 1]] = -inf (n == 1: every token of the row);
 *   bad words: sequence s = bad_tokens[bad_offsets[s] .. bad_offsets[s + 1]) (int32, device; n_bad + 1 ascending offsets), head =
 *     all but its last token: the last token is set to -inf when the head is empty, or len(head) <= R (the length test of 3.0.2's
 *     calc_banned_bad_words_ids against the number of ROWS, kept) and len(head) <= t and the row ends with the head.  A last token
 *     outside [0, V) bans nothing.
 * Every row is processed, finished ones too.  Columns >= V and every word not named above keep their bits.  No atomics: a word
 * has one penalty writer, the bans are idempotent stores behind a barrier.  Needs ld >= V, R >= 1, 1 <= t <= 1024, ld_ids >= t, a
 * finite penalty >= 1, n >= 0, 0 <= n_bad <= 4096 (both tables with n_bad > 0); bad arguments fail with a message and launch nothing. */
int kmb_logits_process(float* logits, int ld, int V, int R, const int64_t* ids, int ld_ids, int t, float repetition_penalty,
                       int no_repeat_ngram_size, const int32_t* bad_tokens, const int32_t* bad_offsets, int n_bad, void* stream);
/* The decode loop's form of kmb_logits_process on the logits the last kmb_gen_step wrote (V and R are the handle's; needs kmb_gen_begin
 * with num_beams == 1): the same edit.  When `logits` are the ones that step's statistics were taken for, the statistics are dropped
 * (kmb_gen_stats_blocks() == 0 afterwards): they describe the unedited logits.  The embedding a later kmb_gen_greedy_step /
 * kmb_gen_sample_step folds in is not affected. */
int kmb_gen_logits_process(kmb_handle* h, float* logits, int ld, const int64_t* ids, int ld_ids, int t, float repetition_penalty,
                           int no_repeat_ngram_size, const int32_t* bad_tokens, const int32_t* bad_offsets, int n_bad, void* stream);
/* CIDEr / CIDEr-D over TOKEN IDS as a sequence-level reward (self-critical training): out[b] (fp32 [B], device) = the score of row b
 * of ids [B, ld] (int64, device, L columns read) against the references of item item_of_row[b] (int32 [B], device).  ONE launch, one
 * workgroup per row, stateless, no host synchronisation.  Not the word-level metric of the reference's evaluation: tokens are ids.
 * Tokens of a row: column 0 (the decoder start token) is skipped, the row stops in front of the first eos_token behind it, every
 * pad_token and bos_token is dropped (and any id outside [0, 65536)).  With g_x,n(w) = count_x(w) * idf_n(w) over the n-grams w of
 * order n = 1..4:  s_n(h, r) = sum_{w in h} num / (||g_h,n|| ||g_r,n||), 0 when a norm is 0, num = min(g_h, g_r) * g_r (variant 0,
 * CIDEr-D) or g_h * g_r (variant 1, plain CIDEr); pen = exp(-(L_h - L_r)^2 / (2 sigma^2)) (variant 0) or 1;
 * score = (10 / m) sum_r pen * 1/4 sum_n s_n over the item's m references.  An item index outside [0, n_items), an item without
 * references and an empty hypothesis score 0 and read no table.
 * The tables (src/rewards.py build_cider_tables; device memory except df_offsets, 5 int64 on the HOST, read at the call): an n-gram
 * is the key sum_k tok[k] << 16 (n - 1 - k), one key space per order, ordered UNSIGNED (int64 bit patterns);
 *   df_keys / df_idf [df_offsets[4]]: order n's distinct n-grams in [df_offsets[n - 1], df_offsets[n]), ascending, with
 *     idf = log N - log max(1, df); idf_miss = float32(log N) for an n-gram in no reference;
 *   item_ref_offsets [n_items + 1]; ref_len [n_refs]; ref_norm [n_refs, 4] = ||g_r,n||;
 *   ref_ng_offsets [4 n_refs + 1]: slice 4 r + (n - 1) of ref_keys (ascending) / ref_w (count * idf), n_ref_entries in all.
 * Lookups are binary searches; fp32, no atomics, fixed reduction order: the same input gives the same bits.  Needs
 * 1 <= L <= 256 (KMB_CIDER_MAX_T, csrc/cider_reward.h), ld >= L, B >= 0, sigma finite and > 0, variant 0 or 1 and no null
 * pointer; fails with a message and launches nothing otherwise. */
int kmb_cider_reward(const int64_t* ids, int ld, int B, int L, int pad_token, int bos_token, int eos_token, const int32_t* item_of_row,
                     int n_items, const int64_t* df_keys, const float* df_idf, const int64_t* df_offsets, float idf_miss,
                     const int32_t* item_ref_offsets, int n_refs, const int32_t* ref_len, const float* ref_norm,
                     const int32_t* ref_ng_offsets, const int64_t* ref_keys, const float* ref_w, int64_t n_ref_entries, int variant,
                     float sigma, float* out, void* stream);
/* One step of greedy beam search with generate()'s score processors (transformers 3.0.2 _generate_beam_search: log_softmax, then
 * postprocess_next_token_scores on the LOG-PROBABILITIES, then + beam score and the 2 * num_beams best per batch item): kmb_beam_step's
 * arguments, outputs and selection, plus kmb_logits_process's processor arguments and the beams' token histories.  At most three
 * launches (the rows' edit sets, kmb_beam_step's two), one when the token is forced; no pass over [R, V] beyond kmb_beam_step's one;
 * stateless.  Per beam row r with tokens ids_in[r * ld_ids + 0 .. t) (int64):
 *   s = log_softmax(logits[r, 0 .. V)), the log-sum-exp of the unedited row -- the edits never renormalise;
 *   repetition_penalty p != 1: every distinct token x of the row once, s[x] = s[x] < 0 ? s[x] * p : s[x] * (1 / p);
 *   -inf at ban_token, at the tokens no_repeat_ngram_size bans and at those the bad words ban (kmb_logits_process's rules, the bad
 *     words' length test against R = B * num_beams rows); a ban wins over a penalty;
 *   + add[r]; per batch item the k best of its num_beams * V scores by (value descending, beam * V + token ascending) into out, and
 *   the next beams as kmb_beam_step chooses them.
 * The selection is exact whatever the edits do to the order: the part launch selects among the unedited tokens only, the combine
 * launch gathers the penalised tokens' logits and merges their scaled scores in.
 * ids_out [B * num_beams, ld_ids] (another buffer than ids_in) receives the next beams' histories:
 * ids_out[i][0 .. t) = ids_in[next_beam_idx[i]][0 .. t), ids_out[i][t] = next_tokens[i].
 * force_token >= 0: kmb_beam_step's forced step (the forced token's log-probability is exactly 0, which the penalty leaves; the
 * caller sees to it that no ban can hit a forced token): no edit, ids_out still advances.
 * Needs kmb_beam_step's shape limits (k <= 16, num_beams <= 16, num_beams * k <= 256, ld % 4 == 0, ld <= 53248), V <= 65536,
 * 1 <= t <= 1024, ld_ids > t, a finite penalty >= 1, n >= 0, 0 <= n_bad <= 4096 and scratch of
 * kmb_beam_step_processed_scratch(B * num_beams, t, n_bad) floats; bad arguments fail with a message and launch nothing. */
int64_t kmb_beam_step_processed_scratch(int rows, int t, int n_bad);
int kmb_beam_step_processed(const float* logits, int ld, int V, int B, int num_beams, const float* add, int force_token, int ban_token,
                            int k, int32_t* out, int eos_token, float* next_scores, int64_t* next_tokens, int32_t* next_beam_idx,
                            float* scratch, int64_t scratch_floats, const int64_t* ids_in, int64_t* ids_out, int ld_ids, int t,
                            float repetition_penalty, int no_repeat_ngram_size, const int32_t* bad_tokens, const int32_t* bad_offsets,
                            int n_bad, void* stream);
/* The decode loop's form of kmb_beam_step_processed on the logits the last kmb_gen_step wrote (V and B are the handle's), with
 * kmb_gen_beam_step's reorder_step contract: reorder_step >= 0 also reorders the caches by next_beam_idx in the same launch and
 * usually embeds next_tokens for step reorder_step + 1 (kmb_gen_embedded_step tells; kmb_gen_step(h, NULL, ...) uses them).  It never
 * selects from the vocabulary projection's statistics (an edit can invalidate the block maxima their threshold comes from) and
 * leaves them as they are: the logits are not edited. */
int kmb_gen_beam_step_processed(kmb_handle* h, const float* logits, int ld, int num_beams, const float* add, int force_token, int ban_token,
                                int k, int32_t* out, int eos_token, float* next_scores, int64_t* next_tokens, int32_t* next_beam_idx,
                                float* scratch, int64_t scratch_floats, const int64_t* ids_in, int64_t* ids_out, int ld_ids, int t,
                                float repetition_penalty, int no_repeat_ngram_size, const int32_t* bad_tokens, const int32_t* bad_offsets,
                                int n_bad, int reorder_step, void* stream);
/* One decode step of beam sampling (generate(do_sample=True, num_beams > 1): transformers 3.0.2 _generate_beam_search, sampling
 * branch, reached from the reference's --num_beams with --do_sample, src/generation.py:22-32), two launches, stateless
 * like kmb_beam_step.  Per row r = b * num_beams + j of logits [B * num_beams, ld] (fp32, V real columns, NaN read as -inf):
 * s = log_softmax(row), s[ban_token] = -inf after the normalisation (-1: none; the min_length EOS ban), s += add[r] (NULL: 0),
 * s /= temperature (correctly rounded, skipped at 1); top_k > 0: remove s < the min(max(top_k, 2), V)-th largest score (ties
 * stay); top_p < 1: ranked by (score descending, index ascending), keep the first three and every token whose softmax mass
 * ranked before it is <= top_p.  Per batch item, k = 2 * num_beams draws without replacement over its num_beams * V filtered
 * scores -- torch.multinomial(softmax, k): the k largest s - log(noise), noise [B, ld_noise] fp32 Exp(1) draws supplied by the
 * caller (column j * V + token, read at kept tokens only), exact ties to the lower column -- sorted by score descending (ties
 * keep the draw order) into out [B, k, 2] int32 {score bits, j * V + token} (kmb_beam_step's layout); next_scores /
 * next_tokens / next_beam_idx [B * num_beams]: the first num_beams of them whose token is not eos_token (-1: none), as
 * kmb_beam_merge_select.  Needs k == 2 * num_beams <= 16, 1 <= V <= 65536, ld >= V, ld_noise >= num_beams * V,
 * 0 < temperature, 0 < top_p <= 1 and scratch of kmb_beam_sample_scratch(B * num_beams) floats (device; each row's draws
 * between the two launches, a per-row stage and a per-item merge); fails with a message and launches nothing otherwise.
 * Deterministic: integer atomics only. */
int kmb_beam_sample_step(const float* logits, int ld, int V, int B, int num_beams, const float* add, float temperature, int top_k,
                         float top_p, int ban_token, const float* noise, int ld_noise, int k, int32_t* out, int eos_token,
                         float* next_scores, int64_t* next_tokens, int32_t* next_beam_idx, float* scratch, int64_t scratch_floats,
                         void* stream);
int64_t kmb_beam_sample_scratch(int rows);
/* The decode loop's form of kmb_beam_sample_step on the logits the last kmb_gen_step wrote (V and B are the handle's), with
 * kmb_gen_beam_step's reorder_step contract: reorder_step >= 0 also reorders the caches by next_beam_idx in the same launch and
 * usually embeds next_tokens for step reorder_step + 1 (kmb_gen_embedded_step tells; kmb_gen_step(h, NULL, ...) uses them). */
int kmb_gen_beam_sample_step(kmb_handle* h, const float* logits, int ld, int num_beams, const float* add, float temperature, int top_k,
                             float top_p, int ban_token, const float* noise, int ld_noise, int k, int32_t* out, int eos_token,
                             float* next_scores, int64_t* next_tokens, int32_t* next_beam_idx, float* scratch, int64_t scratch_floats,
                             int reorder_step, void* stream);
int64_t kmb_gen_workspace_bytes(const kmb_handle* h, int B, int S, int num_beams, int max_length, int n_features);
/* The format of the six per-layer decoder matrices the fused decode blocks read (KMB_WFMT_BF16, the default, or
 * KMB_WFMT_FP8_E4M3: KmbDecodeBlock.w_format).  State of the handle, read by the kmb_gen_* family only: kmb_gen_workspace_bytes
 * sizes the packed copies for it (FP8: half the bytes plus the row exponents), the next kmb_gen_begin packs in it, kmb_gen_step
 * hands it to the blocks; training, scoring and the vocabulary projection never see it.  FP8 exists only where the fused blocks
 * run: this call refuses it for a configuration they do not take, and kmb_gen_begin refuses it for more than 1024 rows, under
 * KMB_GEN_FUSED=0 and in the fp32 validation mode -- never a silent bf16 decode.  Ends the active generation. */
int kmb_gen_set_weight_format(kmb_handle* h, int format);

/* Data-parallel runs share the GPU between the GEMMs and RCCL's all-reduce kernel (reference: torch DDP's NCCL streams,
 * vcg_train.py:98).  The persistent GEMM variants keep one workgroup per CU; with on != 0 they hand out EVERY tile through
 * an atomic counter, so workgroups that cannot be placed while the communication kernel holds CUs leave no work behind.
 * Process-wide; results do not depend on it. */
int kmb_gemm_shared_device(int on);

/* Diagnostic: what kmb_op_gemm would do with *p, decided exactly as the launch decides it -- no GPU call, the operands
 * are never dereferenced (any aligned non-null addresses do).  forced_variant > 0: as under KMB_GEMM_VARIANT=forced_variant;
 * 0: the library's own choice.  out[0] = 0: one triple follows, the launch itself; out[0] = 1: the first launch of this
 * shape times candidates, one triple each in the tuner's order.  A triple is (configuration = variant | tile order << 4
 * (variant 0: the narrow kernel), kernel variant that runs it (honours kmb_gemm_shared_device), tile_order it is launched
 * with).  Returns the number of int32 words written, -1 for a problem kmb_op_gemm refuses or a cap too small. */
int kmb_debug_gemm_route(const KmbGemm* p, int forced_variant, int32_t* out, int32_t cap);

/* Diagnostic: the kernel kmb_op_decode_block would run for *p, decided by the function the launch itself asks -- no GPU call, the
 * operands are never dereferenced.  Kind 0: the wide projection (two 16-column tiles per wave, N >= 1536) or the one-tile projection with
 * 2 / 4 / 6 staged 16-byte chunks per lane (K = 768 | 1536 | 2304, 3072); kind 1: the self-attention block; kind 2: the vector
 * cross-attention block, or the one that stages each batch item's keys / values in LDS and runs on the matrix cores (kv_group >= 4,
 * Tk <= 120 and 160 KB of LDS: Tk <= 104 at K = 768).  Returns -1 for a block kmb_op_decode_block refuses. */
#define KMB_DECODE_ROUTE_PROJ_WIDE 0
#define KMB_DECODE_ROUTE_PROJ2 1
#define KMB_DECODE_ROUTE_PROJ4 2
#define KMB_DECODE_ROUTE_PROJ6 3
#define KMB_DECODE_ROUTE_ATTN_SELF 4
#define KMB_DECODE_ROUTE_ATTN_CROSS 5
#define KMB_DECODE_ROUTE_ATTN_CROSS_KVLDS 6
int kmb_debug_decode_route(const KmbDecodeBlock* p);

/* Diagnostic: the kernel kmb_op_attn_fwd (backward != 0: kmb_op_attn_bwd) would run for *p, answered by the function the launchers themselves
 * ask -- no GPU call, the operands are never dereferenced.  General: one (batch, head) item per workgroup (forward: per item and query tile),
 * any Tq / Tk.  Single-tile: Tq <= 64 and Tk <= 64, persistent over items (forward: from 1024 items on); with Tq, Tk <= 32 and an even head
 * count two heads share a tile.  Query-streaming: Tq > 64, Tk <= 64, not causal -- several targets per input attending to one input's keys
 * (forward of the training step with targets_per_input > 1): persistent over items, K / V staged once per item, the item's query tiles walked
 * with the next tile in flight; at every item count.  The two persistent classes need every tensor below 4 GB.  Returns a negative value for
 * a problem the operator refuses (a backward with Tq > 384 among them, whichever kernel would run it). */
#define KMB_ATTN_ROUTE_GENERAL 0
#define KMB_ATTN_ROUTE_SMALL 1
#define KMB_ATTN_ROUTE_SMALL_PACK 2
#define KMB_ATTN_ROUTE_QSTREAM 3
int kmb_debug_attn_route(const KmbAttn* p, int backward);

/* ================= data parallelism: native RCCL (vcg_train.py:98 DDP, src/utils.py:9-17 init_process_group) =================
 * One process per GPU; the library owns the communicator and a communication stream, and a step's whole gradient
 * exchange is ONE call: every gradient bucket (kmb_bucket_range, backward completion order) is reduced on the
 * communication stream behind that bucket's completion event of kmb_backward, in pieces of at most max_piece_elems,
 * so the collectives overlap the rest of backward; with `adamw` set each piece's fused optimizer update is chained
 * right behind its collective on the same stream.  Semantics = torch DistributedDataParallel's: after the call every
 * rank holds the arithmetic MEAN over ranks of the per-rank gradients.  The communicator is bootstrapped with a
 * 128-byte id made by rank 0 (kmb_comm_unique_id) and handed to the other ranks by any host channel. */
#define KMB_COMM_ID_BYTES 128
int kmb_comm_unique_id(void* id_host);                                   /* ncclGetUniqueId: call on rank 0 */
int kmb_comm_init(kmb_handle* h, int rank, int world, const void* id_host);   /* ncclCommInitRank on the current device */
int kmb_comm_destroy(kmb_handle* h);
int kmb_comm_info(const kmb_handle* h, int32_t* rank, int32_t* world);   /* world 0: no communicator */
/* parameters and final_logits_bias of rank `root` to every rank (DDP's broadcast at wrap time), bf16 mirror refreshed */
int kmb_comm_broadcast_params(kmb_handle* h, int root, void* stream);
typedef struct kmb_allreduce_opts {
  int32_t algo;               /* 0: ncclAllReduce(avg) per piece; 1: ncclReduceScatter(avg) -> [AdamW on this rank's shard ->
                               * ncclAllGather of the updated parameters] (ZeRO-1 form: optimizer traffic / world; moments are
                               * valid on the owning rank only until kmb_comm_gather_moments); world must divide 8 */
  int32_t after_compute;      /* 1: the communication stream first waits for everything already enqueued on compute_stream */
  int64_t max_piece_elems;    /* <= 0: 16 Mi elements (64 MB of fp32) */
  const KmbAdamW* adamw;      /* NULL: gradients only (algo 1 then all-gathers the gradients) */
} kmb_allreduce_opts;
int kmb_allreduce_grads(kmb_handle* h, const kmb_allreduce_opts* opts, void* compute_stream);
int kmb_comm_wait(kmb_handle* h, void* compute_stream);                  /* compute_stream waits for the communication stream */
int kmb_comm_gather_moments(kmb_handle* h, void* compute_stream);        /* algo 1: every rank gets every shard's exp_avg / exp_avg_sq */
int64_t kmb_comm_pieces(const kmb_handle* h, int64_t max_piece_elems);   /* number of collectives one kmb_allreduce_grads issues */
/* The partition itself, as a PURE HOST function of the arena layout (no communicator, no device: the world > 1 offsets of
 * kmb_allreduce_grads / kmb_comm_gather_moments come from here and are checked on a CPU, tests/test_comm_plan_cpu.py).
 * Piece i (0 <= i < kmb_comm_pieces) of a `world`-rank exchange as rank `rank` sees it; what DDP's bucket assignment is
 * in the reference (vcg_train.py:98). */
typedef struct kmb_comm_piece {
  int32_t bucket;        /* gradient bucket (kmb_bucket_range) whose completion event the piece waits for */
  int32_t repad_piece;   /* 1: the piece overlaps the image-projection weight (its padded bf16 copy is rebuilt after an update) */
  int32_t repad_shard;   /* 1: this rank's shard does */
  int32_t reserved;
  int64_t offset, count; /* arena range of the piece, in elements; 64-element aligned */
  int64_t shard;         /* count / world, 8-element aligned; 0 when the piece does not split that way (algo 1 refuses it) */
  int64_t mine;          /* offset + rank * shard: the range [mine, mine + shard) this rank reduces / updates / owns moments of */
} kmb_comm_piece;
int kmb_comm_plan(const kmb_handle* h, int world, int rank, int64_t max_piece_elems, int64_t i, kmb_comm_piece* out);
/* 1 after an algo-1 exchange with a fused optimizer on more than one rank (exp_avg / exp_avg_sq current on the owning
 * rank's shards only), 0 again after kmb_comm_gather_moments */
int kmb_comm_moments_sharded(const kmb_handle* h);

/* ================= measurement ================= */
/* time every GEMM launch of the following calls with HIP events on its own stream (bench.py roofline leg);
 * variant = a_kc*2 + b_kc: 3 forward (X W^T), 2 dgrad (dY W), 0 wgrad (dY^T X) */
int kmb_debug_trace(int on);                          /* diagnostic: checksum intermediate buffers of kmb_backward */
int kmb_debug_trace_dump(const char* path);           /* "index layer name checksum" per recorded buffer */
int kmb_set_side_stream(kmb_handle* h, int enable);   /* weight-gradient GEMMs on a side stream (default on) */
int kmb_profile_gemm(int enable);
int kmb_profile_read(int variant, int64_t* launches, double* total_ms, double* total_flops);
int kmb_profile_dump(const char* path);   /* one text line per profiled GEMM launch */
/* out16 (device, zeroed by the caller): per XCD x (s_memtime shader-clock ticks, s_memrealtime 100 MHz ticks) at the point
 * of the stream where it runs; (d ticks / d real) x 100 MHz between two stamps = the clock the chip held in between
 * (bench.py `clock_mhz`: a 3 % box difference shows as clock, not as a regression) */
int kmb_clock_stamp(int64_t* out16, void* stream);

/* The reference's batch carries the region features as a LIST of per-sample [R_i, image_feature_size] fp32 tensors
 * (/root/reference/src/data/collation.py:73-76; /root/reference/src/model/modules.py:24-41 concatenates the non-empty ones).
 * rows_dev_ptrs: HOST array of n DEVICE pointers (entry i may be NULL when rows[i] == 0), rows: HOST array of the R_i.
 * packed_out (device, [sum R_i, feat_dim] fp32) receives them in list order -- kmb_batch.image_features -- in ceil(n / 128)
 * kernel launches on `stream`, no host synchronisation; the caller keeps the source tensors alive until the stream has passed. */
int kmb_pack_features(const float* const* rows_dev_ptrs, const int32_t* rows, int32_t n, int32_t feat_dim, float* packed_out,
                      void* stream);

/* ================= single operators (unit tests / profiling) ================= */
int kmb_op_gemm(const KmbGemm* p, void* stream);
/* the same product on the "all rows" kernel (one workgroup per 256 output columns holds every row: M <= 320, forward layout, bias
 * only, fp32 output): what a generation decode step's vocabulary projection runs; bit-identical to kmb_op_gemm */
int kmb_op_gemm_allrows(const KmbGemm* p, void* stream);
/* ... and its statistics epilogue: stats[(row * blocks + blk) * 2] = max, [... + 1] = sum of exp(v - max) over the
 * 256 columns of block blk, blocks = ceil(N / 256) (kmb_op_gemm_allrows_stats_floats(N) floats); kmb_beam_step_stats is kmb_beam_step selecting from them
 * (stats_blocks = ceil(V / 256); what kmb_gen_step + kmb_gen_beam_step run) */
int64_t kmb_op_gemm_allrows_stats_floats(int N);
int kmb_op_gemm_allrows_stats(const KmbGemm* p, float* stats, void* stream);
/* the vocabulary projection's SCORING class (what kmb_score's store-free head runs): C = A B^T + bias is never stored;
 * stats[(row * (N / 64) + col / 64) * 2] = the maximum of the row's 64 values in that column block, [... + 1] = the sum of
 * exp(v - maximum) over them (kmb_op_gemm_score_stats_floats(M, N) floats).  Forward layout (a_kc = b_kc = 1), M and N multiples of
 * 256 with at least 128 tiles of 256 x 256, K a multiple of 64 and >= 320, bias required, every output / epilogue field of *p unset. */
int64_t kmb_op_gemm_score_stats_floats(int M, int N);
int kmb_op_gemm_score(const KmbGemm* p, float* stats, void* stream);
/* ... and its finish: token_logprob[r] = label_logit[r] - logsumexp(row r's `blocks` pairs) (0 where labels[r] is -100 or outside
 * [0, V)), then per batch item the sum of -token_logprob and the number of valid rows over its T rows, in row order */
int kmb_op_score_rows_finish(const float* stats, int blocks, const float* label_logit, const int64_t* labels, int B, int T, int V,
                             float* token_logprob, float* sample_nll, int32_t* sample_count, void* stream);
int kmb_beam_step_stats(const float* logits, int ld, int V, int B, int num_beams, const float* add, int force_token, int ban_token,
                        int k, int32_t* out, int eos_token, float* next_scores, int64_t* next_tokens, int32_t* next_beam_idx,
                        const float* stats, int stats_blocks, void* stream);
/* n (1 .. 8) independent weight-gradient products dW_i = dY_i^T X_i (both operands token-major, fp32 output, no split-K) as ONE
 * launch walking all their 128 x 128 tiles: what kmb_backward issues per layer when the batch is short (<= 3072 tokens: `group_tokens`,
 * csrc/engine_train.cpp::backward_impl; torch
 * autograd's per-Linear weight gradients behind the reference's loss.backward(), src/training.py:55-59, 138-142); every output
 * bit-identical to the same problem through kmb_op_gemm */
int kmb_op_gemm_group(const KmbGemm* probs, int32_t n, void* stream);
int kmb_op_attn_fwd(const KmbAttn* p, void* stream);
int kmb_op_attn_bwd(const KmbAttn* p, void* stream);
int kmb_op_attn_decode(const KmbAttnDecode* p, void* stream);
int kmb_op_decode_block(const KmbDecodeBlock* p, void* stream);
/* packed <- W ([N, K] row-major, row stride ld; N % 16 == 0, K % 64 == 0) in the order KmbDecodeBlock.W is read */
int kmb_op_decode_pack(const kmb_bf16* W, int ld, int N, int K, kmb_bf16* packed, void* stream);
/* The FP8 (e4m3) form of W for KmbDecodeBlock.w_format == KMB_WFMT_FP8_E4M3: exps[n] = the smallest integer e with
 * max_k |W[n, k]| * 2^-e <= 448 (over the row's finite elements; clamped to [-120, 119]; 0 for a zero row), codes = W * 2^-exps[n]
 * rounded to nearest even into OCP e4m3fn (subnormal codes kept; saturated at +-448 where the exponent was clamped and for
 * infinities; a NaN becomes the NaN code), N * K bytes in the order the block reads them: one KiB per (16-row tile n, 64-deep
 * chunk c), lane l's 16 bytes = W[n*16 + (l & 15)][c*64 + (l >> 4)*16 .. + 15].  N % 16 == 0, K % 64 == 0, ld >= K. */
int kmb_op_decode_pack_fp8(const kmb_bf16* W, int ld, int N, int K, uint8_t* codes, int8_t* exps, void* stream);
int kmb_abi_sizeof_decode_block(void);
int kmb_op_ln_fwd(const kmb_bf16* z, const float* gamma, const float* beta, kmb_bf16* y, float* mean, float* rstd,
                  int M, int D, float eps, void* stream);
/* partials: device float scratch of kmb_op_ln_bwd_scratch(M, D) floats */
int64_t kmb_op_ln_bwd_scratch(int M, int D);
int kmb_op_ln_bwd(const kmb_bf16* dy, const kmb_bf16* z, const float* mean, const float* rstd, const float* gamma,
                  kmb_bf16* dz, kmb_bf16* out2, const KmbDrop* dy_drop, const KmbDrop* out2_drop, float* dgamma,
                  float* dbeta, float* scratch, int M, int D, void* stream);
/* Test entry points of the row kernels between the GEMMs (tests/test_row_kernels_gpu.py).  Each refuses, with a message, what its
 * kernel cannot take: a null required pointer, a misaligned one, a ragged width or stride.
 * kmb_op_ln_bwd_sub: kmb_op_ln_bwd reduced as a training step reduces it, in ONE launch: dgamma | dbeta are one 2 D-wide output
 * (dbeta == dgamma + D, as in the gradient arena), dsub [D] receives the kernel's third partial: the column sums of the sub-layer
 * gradient (of out2's fp32 values under out2_drop when out2 is given, of dz's otherwise; summed before the bf16 rounding). */
int kmb_op_ln_bwd_sub(const kmb_bf16* dy, const kmb_bf16* z, const float* mean, const float* rstd, const float* gamma,
                      kmb_bf16* dz, kmb_bf16* out2, const KmbDrop* dy_drop, const KmbDrop* out2_drop, float* dgamma,
                      float* dbeta, float* dsub, float* scratch, int M, int D, void* stream);
/* y = LayerNorm(bf16((slab 0 + slab 1 + ... in slice order) + bias + residual)); slabs [nslabs][stride] floats, rows of D; bias may be
 * NULL, residual is required; D % 8 == 0, D <= 1024, stride % 4 == 0, ld_res % 8 == 0 */
int kmb_op_ln_fwd_slabs(const float* slabs, int nslabs, int64_t stride, const float* bias, const kmb_bf16* residual, int ld_res,
                        const float* gamma, const float* beta, kmb_bf16* y, int M, int D, float eps, void* stream);
/* out[i] = beta * out[i] + slab 0 [i] + slab 1 [i] + ... (slice order); n % 4 == 0 (fp32 out), n % 8 == 0 (bf16 out), stride % 4 == 0 */
int kmb_op_reduce_slabs(const float* slabs, int nslabs, int64_t stride, float* out, int64_t n, float beta, void* stream);
int kmb_op_reduce_slabs_bf16(const float* slabs, int nslabs, int64_t stride, kmb_bf16* out, int64_t n, void* stream);
/* out[r][c] = bf16(drop((sum of the slabs + bias[c]) * (c < col_scale_n ? col_scale : 1)) + residual[r][c]); bias, drop and residual
 * may be NULL; the mask is kmb_op_dropout_mask(seed, thr16 / 65536, M, N); N, ld_res and ld_out multiples of 8 */
int kmb_op_reduce_slabs_epi(const float* slabs, int nslabs, int64_t stride, const float* bias, float col_scale, int col_scale_n,
                            const KmbDrop* drop, const kmb_bf16* residual, int ld_res, kmb_bf16* out, int ld_out, int M, int N,
                            void* stream);
int64_t kmb_op_colsum_scratch(int M, int N);
int kmb_op_colsum(const kmb_bf16* X, int ld, int M, int N, float* out, float* scratch, void* stream);
int kmb_op_img_rowmap(const int64_t* ids, const int32_t* feat_off, int B, int S, int64_t img_feat_id, int64_t cls_id,
                      int32_t* img_src, int32_t* status, void* stream);
int kmb_op_cast_pad(const float* x, int N, int Fin, kmb_bf16* y, int Fpad, void* stream);
int kmb_op_embed_ln_fwd(const int64_t* ids, const int32_t* img_src, const float* E, const float* img_emb,
                        const float* P, int pos_base, int S, float scale, const float* gamma, const float* beta,
                        kmb_bf16* z, kmb_bf16* y, float* mean, float* rstd, int M, int D, float eps,
                        const KmbDrop* drop, void* stream);
int kmb_op_embed_bwd(const kmb_bf16* dz, const int64_t* ids, const int32_t* img_src, float scale, float* dE,
                     kmb_bf16* dimg, int64_t pad_id, int M, int D, void* stream);
int kmb_op_pos_bwd(const kmb_bf16* dz, int B, int S, int D, float* dP, int pos_base, int P_rows, void* stream);
int kmb_op_ce(const float* logits, int ldv, int V, const int64_t* labels, int rows, float grad_scale,
              float* loss_rows, kmb_bf16* dlogits, int32_t* count, float* loss, void* stream);
/* the same on bf16 logits (the training head; ldv % 8 == 0, ldv <= 65536): dlogits may be NULL or equal to logits (the gradient then
 * replaces the logits in place); status (optional, device int32): bit 1 is set when a label is neither -100 nor in [0, V) */
int kmb_op_ce_bf16(const kmb_bf16* logits, int ldv, int V, const int64_t* labels, int rows, float grad_scale, float* loss_rows,
                   kmb_bf16* dlogits, int32_t* count, float* loss, int32_t* status, void* stream);
/* count[0] = number of labels in [0, V); status as above */
int kmb_op_count_valid(const int64_t* labels, int n, int V, int32_t* count, int32_t* status, void* stream);
/* loss[0] = sum(loss_rows[0, rows)) / count[0], NaN when count[0] == 0 (torch's mean over no targets) */
int kmb_op_loss_finish(const float* loss_rows, int rows, const int32_t* count, float* loss, void* stream);
/* The tied head's cross-entropy without a pass over the logits (KmbGemm act 5), piece by piece.
 * shift[r] = H[r] . E[labels[r]] + bias[labels[r]] (1e30 where the label is -100 or out of range); bias_pad[0, V) = bias, [V, Vpad) = -1e30 */
int kmb_op_ce_label_logit(const kmb_bf16* H, int ldh, const kmb_bf16* E, int lde, const float* bias, const int64_t* labels, int rows,
                          int d, int V, int Vpad, float* shift, float* bias_pad, void* stream);
/* per row, from the act 5 GEMM's row_sums: srow = S, loss_rows = log S - pick (pick NULL: 0), alpha = lm_factor / (count[0] S),
 * ah = bf16(alpha H) (optional, [rows, d]), P[r][label] := bf16(exp(pick) - S) (P optional); ignored rows: all zero */
int kmb_op_ce_rows_finish(const float* row_sums, int ld_sums, int nparts, const float* pick, const int64_t* labels, const int32_t* count,
                          float lm_factor, int rows, int d, int V, const kmb_bf16* H, int ldh, float* loss_rows, float* srow,
                          float* alpha, kmb_bf16* ah, kmb_bf16* P, int ldp, void* stream);
/* out[r] = bf16(alpha[r] * sum over s < nslabs of slab[s * stride + r * d ...]) */
int kmb_op_ce_dgrad_finish(const float* slab, int nslabs, int64_t stride, const float* alpha, kmb_bf16* out, int rows, int d, void* stream);
/* Label smoothing (kmb_set_label_smoothing), piece by piece.  With eps = 0 each of these leaves the bits of its counterpart above.
 * kmb_op_ce_smooth / kmb_op_ce_bf16_smooth: loss_rows[r] = lse - (1 - eps) logit[label] - eps mean_{j < V} logit[j],
 * dlogits = (softmax - (1 - eps) onehot - eps / V) grad_scale / count, rounded once; pad columns and ignored rows stay zero. */
int kmb_op_ce_smooth(const float* logits, int ldv, int V, const int64_t* labels, int rows, float grad_scale, float eps,
                     float* loss_rows, kmb_bf16* dlogits, int32_t* count, float* loss, void* stream);
int kmb_op_ce_bf16_smooth(const kmb_bf16* logits, int ldv, int V, const int64_t* labels, int rows, float grad_scale, float eps,
                          float* loss_rows, kmb_bf16* dlogits, int32_t* count, float* loss, int32_t* status, void* stream);
/* wsum[0, d) = sum_{j < V} E[j] in fp32, wsum[d] = sum_{j < V} bias[j] (wsum: d + 8 floats; d, lde multiples of 8).  Deterministic: workgroups
 * leave partial rows in scratch (kmb_op_ce_vocab_sum_scratch(V, d) floats), one pass sums them in a fixed order. */
int64_t kmb_op_ce_vocab_sum_scratch(int V, int d);
int kmb_op_ce_vocab_sum(const kmb_bf16* E, int lde, const float* bias, int V, int d, float* wsum, float* scratch, void* stream);
/* kmb_op_ce_rows_finish with smoothing: shift (required) is kmb_op_ce_label_logit's; wsum as above.  loss_rows = log S - pick +
 * eps (shift - (H . wsum + wsum[d]) / V), P[r][label] := bf16(exp(pick) - (1 - eps) S), beta[r] = eps lm_factor / (count[0] V) on valid rows
 * (0 elsewhere), neg_u[0, d) = -sum_r beta[r] H[r] (optional, with scratch of kmb_op_ce_rows_finish_smooth_scratch(rows, d) floats:
 * per-workgroup partial sums, finished in a fixed order).  H is always required here. */
int64_t kmb_op_ce_rows_finish_smooth_scratch(int rows, int d);
int kmb_op_ce_rows_finish_smooth(const float* row_sums, int ld_sums, int nparts, const float* pick, const float* shift, const int64_t* labels,
                                 const int32_t* count, float lm_factor, float eps, int rows, int d, int V, const kmb_bf16* H, int ldh,
                                 const float* wsum, float* loss_rows, float* srow, float* alpha, float* beta, kmb_bf16* ah, kmb_bf16* P,
                                 int ldp, float* neg_u, float* scratch, void* stream);
/* out[r] = bf16(alpha[r] * sum over s < nslabs of slab[s * stride + r * d ...] - beta[r] * wsum): one rounding */
int kmb_op_ce_dgrad_finish_smooth(const float* slab, int nslabs, int64_t stride, const float* alpha, const float* beta, const float* wsum,
                                  kmb_bf16* out, int rows, int d, void* stream);
/* Per-row loss weights (kmb_forward_opts.row_weights / loss_reduction), piece by piece.  weights: [rows] fp32 or NULL; reduction 0 mean,
 * 1 sum.  loss_rows[r] and the row's gradient factor are multiplied by weights[r] (read only in rows with a valid label); with reduction 1
 * the denominator is 1 (0 without a valid label) and loss[0] the plain sum.  `count` holds TWO words here: count[0] the number of valid
 * labels, count[1] the 0 / 1 denominator word that reduction 1 uses.  eps = 0 runs the plain instance, eps > 0 the label-smoothing one.
 * NULL weights with reduction 0 launch what kmb_op_ce / kmb_op_ce_bf16 / kmb_op_ce_rows_finish (or their _smooth forms) launch. */
int kmb_op_ce_weighted(const float* logits, int ldv, int V, const int64_t* labels, int rows, float grad_scale, float eps,
                       const float* weights, int reduction, float* loss_rows, kmb_bf16* dlogits, int32_t* count, float* loss, void* stream);
int kmb_op_ce_bf16_weighted(const kmb_bf16* logits, int ldv, int V, const int64_t* labels, int rows, float grad_scale, float eps,
                            const float* weights, int reduction, float* loss_rows, kmb_bf16* dlogits, int32_t* count, float* loss,
                            int32_t* status, void* stream);
/* kmb_op_ce_rows_finish (eps = 0: shift, wsum, beta, neg_u and scratch are not used and may be NULL) or kmb_op_ce_rows_finish_smooth
 * (eps > 0) with weights: loss_rows, alpha, the a . H copy, beta and neg_u carry weights[r]; srow and the label's entry of P do not.
 * count[0] is the caller's (kmb_op_count_valid); with reduction 1 the entry writes count[1] and divides by it. */
int kmb_op_ce_rows_finish_weighted(const float* row_sums, int ld_sums, int nparts, const float* pick, const float* shift,
                                   const int64_t* labels, int32_t* count, float lm_factor, float eps, const float* weights, int reduction,
                                   int rows, int d, int V, const kmb_bf16* H, int ldh, const float* wsum, float* loss_rows, float* srow,
                                   float* alpha, float* beta, kmb_bf16* ah, kmb_bf16* P, int ldp, float* neg_u, float* scratch, void* stream);
/* out[M, N] (fp32) = beta * out + sum over s < nslabs of slabs[s * stride ...] + rowvec[column]: the slab reduction of a split weight
 * gradient with a row vector added to every row (the tied matrix's -u); M * N and stride multiples of 4, N a multiple of 4 */
int kmb_op_reduce_slabs_rowvec(const float* slabs, int nslabs, int64_t stride, float* out, int M, int N, float beta, const float* rowvec,
                               void* stream);
/* pre-training heads (csrc/heads.hip).  loss_rows[r] = KL(target[r] || softmax(logits[r, :C])); dlogits (optional, bf16, row stride
 * ldd, columns C..ldd-1 zeroed) = (sum(target[r]) softmax - target[r]) grad_scale / rows */
int kmb_op_kl_div(const float* logits, int ld, int C, const float* target, int ldt, int rows, float grad_scale, float* loss_rows,
                  kmb_bf16* dlogits, int ldd, void* stream);
/* dst[i][0, cols) = src[idx[i]][0, cols); cols, src_ld, dst_ld multiples of 8 */
int kmb_op_gather_rows_bf16(const kmb_bf16* src, int src_ld, const int32_t* idx, kmb_bf16* dst, int dst_ld, int rows, int cols,
                            void* stream);
/* The gather with a dropout mask (the two F.dropout calls of a classification head, kmb_set_classif_dropout):
 * dst[i][c] = m(i, c) src[idx_a[i]][c] for c < cols, and, with idx_b != NULL, dst[i][cols + c] = m(i, cols + c) src[idx_b[i]][c] in the same
 * launch (the relation head's object | subject rows).  idx_a == NULL: identity rows -- a matrix masked into another buffer, or in place; idx_b
 * must then be NULL too.  dst == src is refused with an index array (a gather in place would race); otherwise the two must not overlap.  m(row, col) = drop->scale where kmb_op_dropout_mask(drop->seed, drop->thr16 / 65536, rows, written columns) keeps
 * (row, col), +0 elsewhere: the coordinate is the DESTINATION's.  Kept values are multiplied in fp32 and rounded once to bf16.  drop NULL or
 * thr16 == 0: the bits of kmb_op_gather_rows_bf16.  cols, src_ld, dst_ld multiples of 8; dst_ld >= the written columns. */
int kmb_op_gather_rows_drop_bf16(const kmb_bf16* src, int src_ld, const int32_t* idx_a, const int32_t* idx_b, kmb_bf16* dst, int dst_ld,
                                 int rows, int cols, const KmbDrop* drop, void* stream);
/* acc[idx[i]][0, cols) += src[i][0, cols)  (fp32 atomics; acc rows are cols wide) */
int kmb_op_scatter_add_rows(const kmb_bf16* src, int src_ld, const int32_t* idx, float* acc, int rows, int cols, void* stream);
/* y = bf16(float(y) + a), n % 8 == 0 */
int kmb_op_add_f32_into_bf16(kmb_bf16* y, const float* a, int64_t n, void* stream);
/* out[0] = factor * sum(rows[0, n)) / denom */
int kmb_op_mean_rows(const float* rows, int n, float factor, float denom, float* out, void* stream);
int kmb_op_adamw(float* p, const float* g, float* m, float* v, kmb_bf16* p_bf16, int64_t n, const KmbAdamW* hp,
                 void* stream);
/* the clipped / guarded step's three kernels on raw pointers (see kmb_grad_sumsq): partials are doubles, g is 16-byte aligned */
int kmb_op_grad_sumsq(const float* g, int64_t n, float grad_scale, double* partials, int32_t slot0, void* stream);
int kmb_op_grad_sumsq_slots(int64_t n);   /* min(ceil(n / 1024), 1024): a function of n alone */
int kmb_op_clip_finish(const double* partials, int32_t nslots, float max_norm, int32_t skip_nonfinite, const KmbAdamW* hp,
                       KmbStepState* state, void* stream);
int kmb_op_adamw_dev(float* p, const float* g, float* m, float* v, kmb_bf16* p_bf16, int64_t n, const KmbAdamW* hp,
                     const KmbStepState* state, void* stream);
/* gradient accumulation's fold: dst[0, n) = (add ? dst : 0) + src, one rounded add per element; add == 0 never reads dst.  Any 4-byte
 * aligned, non-overlapping ranges */
int kmb_op_grad_fold(float* dst, const float* src, int64_t n, int add, void* stream);
int kmb_op_cast_bf16(const float* x, kmb_bf16* y, int64_t n, void* stream);
/* keep[i] = 1 if the dropout generator keeps element (row, col) for this site seed / probability */
int kmb_op_dropout_mask(uint32_t seed, float p, int rows, int cols, uint8_t* keep, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* KMBART_H */
