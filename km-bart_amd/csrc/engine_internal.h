// What the engine's translation units share: the handle, the workspace layouts, the error plumbing and the helpers that cross files.
//   engine.cpp        create / destroy, parameter census, bind, settings, status, GEMM dispatch, stream plumbing, profiler, trace
//   engine_train.cpp  training layout, forward / backward, the LM head, kmb_score, the hidden-state / attention readers
//   engine_comm.cpp   kmb_comm_*, kmb_allreduce_grads, kmb_adamw_step
//   engine_gen.cpp    generation layout and kmb_gen_*
// Nothing here is part of the C ABI (include/kmbart.h): the namespace is hidden, the library's dynamic symbols stay the exported ones.
#pragma once
#include <hip/hip_runtime.h>
#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include <rccl/rccl.h>
#include "kernels.h"
#include "diag.h"

namespace kmbi __attribute__((visibility("hidden"))) {

int fail(const char* fmt, ...);   // sets kmb_last_error's text (thread-local, engine.cpp), returns 1
#define HIPCHK(expr)                                                                       \
  do {                                                                                     \
    hipError_t e_ = (expr);                                                                \
    if (e_ != hipSuccess) return fail("%s failed: %s (%s:%d)", #expr, hipGetErrorString(e_), __FILE__, __LINE__); \
  } while (0)
#define KCHK(expr)                 \
  do {                             \
    int rc_ = (expr);              \
    if (rc_ != 0) return rc_;      \
  } while (0)

inline size_t align_up(size_t x, size_t a) { return (x + a - 1) / a * a; }
inline uint64_t splitmix(uint64_t x) {
  x += 0x9E3779B97F4A7C15ull;
  x = (x ^ (x >> 30)) * 0xBF58476D1CE4E5B9ull;
  x = (x ^ (x >> 27)) * 0x94D049BB133111EBull;
  return x ^ (x >> 31);
}

// Thread-local state of one call (defined in engine.cpp; a handle is single-threaded, include/kmbart.h).
// fp32 validation mode (kmb_set_precision): activations are float, the GEMM / attention / LayerNorm / embedding launches
// go to the plain fp32 kernels of fp32_validate.hip.  Activation pointers keep their bf16_t* type in the host code;
// EP() advances them by ELEMENTS of the current width.  Set for the duration of one forward call.
extern __thread bool g_f32;
// split-K slab of the caller's stream for small-batch forward / data-gradient GEMMs (set for the duration of one call)
extern __thread float* g_small_slab;
extern __thread size_t g_small_floats;
inline size_t esz() { return g_f32 ? 4 : 2; }
// KMB_FP32_HEAD=1: fp32 logits + the register-resident fp32 cross-entropy in the bf16 product mode as well.  Read ONCE and
// used by the workspace layout and by the forward pass alike (the logits buffer is sized for whichever head runs).
inline bool force_fp32_head() {
  static const bool on = getenv("KMB_FP32_HEAD") != nullptr && getenv("KMB_FP32_HEAD")[0] == '1';
  return on;
}
template <typename T> inline T* EP(T* p, size_t n) { return (T*)((char*)p + n * esz()); }

struct ParamInfo { std::string name; size_t off; int rows, cols; };
struct AttnP { size_t qkv_w, qkv_b, o_w, o_b, ln_g, ln_b; };
// ca: the cross-attention block; its qkv_w / qkv_b are the QUERY projection only -- the key | value projections of all
// decoder layers live together in the arena (kmb_handle::xkv_w / xkv_b), ca_kv_w / ca_kv_b are this layer's slices
struct LayerP { AttnP sa, ca; size_t ca_kv_w, ca_kv_b, fc1_w, fc1_b, fc2_w, fc2_b, ln_g, ln_b; };
struct Bucket { size_t off, count; };
struct HeadP { size_t dw = 0, db = 0, ow = 0, ob = 0; int d_in = 0, C = 0; bool on = false; };

struct EncAct { bf16_t *qkv, *o, *z1, *y1, *u, *hh, *z2; float *lse, *m1, *r1, *m2, *r2; };
struct DecAct {
  bf16_t *qkv, *o1, *z1, *y1, *cq, *ckv, *o2, *z2, *y2, *u, *hh, *z3;
  float *lse1, *lse2, *m1, *r1, *m2, *r2, *m3, *r3;
};

class Bump {
 public:
  Bump(char* base, size_t cap) : base_(base), cap_(cap), off_(0) {}
  template <typename T> T* take(size_t n) {
    off_ = align_up(off_, 256);
    T* p = reinterpret_cast<T*>(base_ + off_);
    off_ += n * sizeof(T);
    return p;
  }
  // n activation elements of the current precision (bf16, or float in the fp32 validation mode)
  bf16_t* act(size_t n) { return reinterpret_cast<bf16_t*>(take<char>(n * esz())); }
  size_t used() const { return align_up(off_, 256); }
  bool ok() const { return base_ == nullptr || off_ <= cap_; }
 private:
  char* base_; size_t cap_, off_;
};

// What the encoder sub-graph (encoder_forward) reads and writes.  Both layouts hand one out: training has a state buffer and an
// activation set per layer and keeps the embedding's LayerNorm inputs for backward; generation (`shared`) alternates between two
// state buffers, re-uses one activation set for every layer and keeps nothing (ze0 / me0 / re0 null).
struct EncoderBufs {
  int32_t* status; bf16_t* xf; float* img_emb; int32_t* img_src; bf16_t* ze0; float *me0, *re0;
  bf16_t* const* xe; const EncAct* ea; bool shared;
  bf16_t* x(int l) const { return xe[shared ? (l & 1) : l]; }
  const EncAct& act(int l) const { return ea[shared ? 0 : l]; }
};

// gradient buffers read by the weight-gradient GEMMs of the side stream: one per LayerNorm site
// (0 = FFN, 1 = self-attention, 2 = cross-attention) and per layer parity, so that the main stream can run
// up to one layer ahead of the side stream without overwriting what it still reads
// parts[site]: partial sums of the parameter gradients a site reduces (0 FFN LayerNorm, 1 fc1 bias column sums, 2 self-attn
// LayerNorm, 3 self-attn q|k|v bias, 4 cross-attn LayerNorm, 5 cross-attn q|k|v bias): their reducers run on the side
// stream too, so the partials need the same lifetime as the gradient buffers above
// (the cross-attention k | v gradients of every layer go to TrainLayout::dckv_all)
struct BwdBufs { bf16_t *dz[3], *dsub[3], *du, *dqkv, *dcq; float* parts[6]; };

// The training workspace as layout_train (engine_train.cpp) carves it, in carve order.  kmb_workspace_bytes measures with the same code;
// a forward assigns the handle's copy in one struct copy, and backward / the readers use that copy while have_fwd / have_hdec say it is current.
struct TrainLayout {
  int32_t *status = nullptr, *count = nullptr; float* loss_dev = nullptr;
  bf16_t* xf = nullptr; float* img_emb = nullptr; bf16_t* dimg = nullptr; int32_t* img_src = nullptr;
  bf16_t *ze0 = nullptr, *zd0 = nullptr; float *me0 = nullptr, *re0 = nullptr, *md0 = nullptr, *rd0 = nullptr;
  std::vector<bf16_t*> xe, xd;
  std::vector<EncAct> ea; std::vector<DecAct> da;
  bf16_t *ckv_all = nullptr, *dckv_all = nullptr;   // [Me, Ld * 2d]: every decoder layer's cross-attention k | v and their gradients
  float* logits_c = nullptr; size_t logits_c_floats = 0; bf16_t* dlogits_c = nullptr;
  float* slab = nullptr; size_t slab_floats = 0;            // split-K partials of the side stream's weight gradients
  float* small_slab = nullptr; size_t small_floats = 0;     // ... of the small-batch forward / data-gradient GEMMs (caller's stream)
  float* loss_rows = nullptr;
  // tied-head cross-entropy without a pass over the logits (loss.hip): per-row shift / picked label value / row sum / scale,
  // the row-scaled decoder states a . H and the bias padded to Vpad
  float *ce_shift = nullptr, *ce_pick = nullptr, *ce_srow = nullptr, *ce_alpha = nullptr, *ce_bias = nullptr;
  bf16_t* ce_ah = nullptr;
  bf16_t *dhdec = nullptr, *dyA = nullptr, *dyB = nullptr, *dz = nullptr;
  BwdBufs bb[2] = {};
  bf16_t *dob = nullptr, *denc = nullptr;
  float* parts = nullptr;
  float* losses5 = nullptr;
  // pre-training head scratch (null unless heads exist and rows were reserved)
  bf16_t *hx = nullptr, *hy = nullptr, *hdy = nullptr, *hdx = nullptr, *hdlg = nullptr; float *hlg = nullptr, *hloss = nullptr, *dhead = nullptr;
  bf16_t* hyd = nullptr;   // [n, d]: the hidden activations hy under their classif_dropout mask (what out_proj and its weight gradient read)
  float* head_slab = nullptr; size_t head_slab_floats = 0;  // split-K partials of the pre-training heads' weight gradients (caller's stream)
  // label smoothing in the fused head (kmb_set_label_smoothing; loss.hip "Label smoothing as rank-one terms"): wsum | bsum, -u, beta per row and
  // the partial slots of the two deterministic sums (the vocabulary sum's, then the row finish's)
  float *ls_wsum = nullptr, *ls_negu = nullptr, *ls_beta = nullptr, *ls_parts = nullptr;
  EncoderBufs encoder() const { return {status, xf, img_emb, img_src, ze0, me0, re0, xe.data(), ea.data(), false}; }
};

// The generation workspace as layout_gen (engine_gen.cpp) carves it (every pointer starts null)
struct GenLayout {
  int32_t* status = nullptr; bf16_t* xf = nullptr; float* img_emb = nullptr; int32_t* img_src = nullptr;
  bf16_t* xe[2] = {nullptr, nullptr}; EncAct ea{};
  std::vector<bf16_t*> ckv;              // per layer [B*S, 2d]
  std::vector<bf16_t*> kc, vc;           // per layer self caches [R, Tmax, d], addressed through the history index below
  int32_t* kv_row = nullptr;             // [2][R] -> batch item (two copies: kmb_handle::Gen::kv_row is the current one)
  bf16_t *x0 = nullptr, *x1 = nullptr, *qkv = nullptr, *o = nullptr, *z = nullptr, *y = nullptr, *cq = nullptr, *u = nullptr, *hh = nullptr;
  float *mean = nullptr, *rstd = nullptr;
  float* slab = nullptr;   // split-K partial sums of the residual projections of a decode step
  std::vector<bf16_t*> wp;   // per layer: self q|k|v, self out, cross q, cross out, fc1, fc2 in fragment order (decode.hip); empty: not eligible
  std::vector<int8_t*> wexp; // the weight format FP8 e4m3 (kmb_gen_set_weight_format): wp[i] holds codes (half the bytes), wexp[i] the row exponents; else empty
  // History index of the self-attention caches (round 5): position t of beam row r lives in cache row hist[r][t].  A beam reorder
  // (mixins.py:419-434 _reorder_cache) permutes these [R, Tmax] int rows into the other copy instead of gathering every layer's
  // K and V cache ([R, t, d] x 12 buffers: 5-40 us per decode step at batch 64 x 5 beams); the caches are never copied.
  int32_t* hist[2] = {nullptr, nullptr};
  float* head_stats = nullptr;   // the all-rows vocabulary projection's per-block (maximum, sum-exp) pairs (kmb_gen_beam_step)
  EncoderBufs encoder() const { return {status, xf, img_emb, img_src, nullptr, nullptr, nullptr, xe, &ea, true}; }
};

}  // namespace kmbi

struct kmb_handle {
  kmb_config cfg;
  int d, He, Hd, Fe, Fd, V, Vpad, Fin, Fpad, Prows;
  std::vector<kmbi::ParamInfo> params;
  size_t arena = 0;
  size_t img_w, img_b, enc_pos, enc_lne_g, enc_lne_b, dec_pos, dec_lne_g, dec_lne_b, shared;
  // Cross-attention keys and values are projections of the ENCODER output: the same input for every decoder layer, known
  // before the decoder starts.  Their weights [Ld][k | v][d, d] and biases [Ld][k | v][d] are contiguous in the arena so
  // that ONE GEMM computes all layers' keys | values ([Me, Ld * 2d]), ONE data-gradient GEMM (K = Ld * 2d) produces the
  // encoder-output gradient (instead of six launches that each re-read and re-write it) and ONE weight-gradient GEMM
  // their gradients.  Parameter names are the reference's (model.decoder.layers.N.encoder_attn.k_proj.weight ...).
  size_t xkv_w = 0, xkv_b = 0;
  std::vector<kmbi::LayerP> enc, dec;
  kmbi::HeadP head[3];              // mrm, attribute, relation (src/model/model.py:133-158)
  size_t heads_begin = 0, heads_end = 0; int head_rows_cap = 0;
  std::vector<kmbi::Bucket> buckets;   // in backward completion order
  bool enc_given = false;           // the last forward started from the caller's encoder states (kmb_forward_opts)
  std::vector<hipEvent_t> events;
  // bound memory
  float *P = nullptr, *G = nullptr, *M1 = nullptr, *M2 = nullptr, *flb = nullptr;
  bf16_t* PB = nullptr;
  bf16_t* imgw_pad = nullptr;       // inside the bf16 arena tail: [d, Fpad]
  char* ws = nullptr; size_t ws_bytes = 0;
  // the clipped / guarded optimizer step's device record and partial sums (kmb_bind_step_state): the caller's buffer, outside the workspace
  KmbStepState* step_state = nullptr; double* step_partials = nullptr; int step_slots = 0;
  uint64_t seed = 0x5eedULL; uint64_t step = 0;
  bool fp32 = false;    // kmb_set_precision(1): fp32 validation forward
  bool have_hdec = false;   // xd[Ld] of the last forward is still in the workspace (kmb_last_logits)
  int lm_chunk = 8192;  // rows of fp32 logits per LM-head launch (bounds the logits buffer at 1.65 GB for V = 50320)
  // ---- state of the last forward (consumed by backward)
  kmb_batch bt{}; bool have_fwd = false; bool fwd_train = false; bool have_bwd = false;
  int Me = 0, Md = 0, Ntot = 0;
  int tpi = 1;                      // targets per input of the last forward (kmb_forward_opts.targets_per_input): Md = bt.B * tpi * bt.T
  kmbi::TrainLayout tl;             // where the last forward's activations and backward's buffers are
  int32_t* status = nullptr;        // the status word of the last forward / generate (tl.status or gen.L.status): kmb_read_status*
  hipStream_t side = nullptr; bool side_on = true;
  // grouped weight gradients (wgrad_side / wgrad_flush): a layer's problems wait here until the layer's last one is known
  std::vector<KmbGemm> wg_pending; bool wg_group = false;
  std::vector<hipEvent_t> ring; size_t ring_pos = 0;
  std::vector<hipEvent_t> layer_done;   // recorded on the side stream
  hipEvent_t head_wgrad_done = nullptr; bool head_wgrad_pending = false;
  // ---- native data parallelism (kmb_comm_*)
  ncclComm_t comm = nullptr; int comm_rank = 0, comm_world = 0;
  hipStream_t comm_stream = nullptr; hipEvent_t comm_ev = nullptr;
  int64_t comm_piece_cap = 0;   // piece size of the last algo-1 exchange: the moments' shards follow its piece boundaries
  uint64_t mirror_version = 1;   // bumped whenever the bf16 mirror is rewritten (sync / optimizer): kmb_gen_begin repacks the decoder weights only then
  bool moments_sharded = false; // set by an algo-1 exchange with a fused optimizer on more than one rank, cleared by kmb_comm_gather_moments
  hipEvent_t next_event() { hipEvent_t e = ring[ring_pos]; ring_pos = (ring_pos + 1) % ring.size(); return e; }   // (order_behind only)
  // ---- generation state: the layout of the last kmb_gen_begin and what the decode steps change
  struct Gen {
    bool active = false; int B = 0, S = 0, nb = 0, R = 0, Tmax = 0;
    kmb_batch bt{};
    kmbi::GenLayout L;                     // (kmb_gen_greedy_step / kmb_gen_sample_step may swap L.x0 and L.x1)
    int32_t* kv_row = nullptr;             // [R] -> batch item: the current one of the two copies at L.kv_row
    // the last kmb_gen_step's final decoder states: normalised rows at last_x, or (fused blocks, no vocabulary projection)
    // pre-LayerNorm sums at last_z with the last layer's LayerNorm (last_g, last_b) still to be applied
    const bf16_t* last_x = nullptr; const bf16_t* last_z = nullptr; const float *last_g = nullptr, *last_b = nullptr;
    int hcur = 0;                          // the current one of L.hist's two copies
    // per-block (maximum, sum-exp) pairs the last kmb_gen_step's vocabulary projection left in L.head_stats beside the logits at head_stats_for
    // (head_stats_blocks column blocks; 0: none -- the step ran another GEMM kernel, or no projection): kmb_gen_beam_step selects from them
    int head_stats_blocks = 0; const float* head_stats_for = nullptr;
    // x0 already holds the embedded rows of decode step x0_step (the step entry point that chose the tokens embedded them in its own launch): a
    // kmb_gen_step(tokens = NULL) of exactly that step uses them instead of embedding.  -1: nothing pending
    int x0_step = -1;
    uint64_t packed_version = 0; const bf16_t* packed_at = nullptr;   // the fragment-order copies at L.wp[0] were made from mirror version ...
    int packed_format = 0;                 // ... in this weight format
    int w_format = 0;                      // KMB_WFMT_* (kmb_gen_set_weight_format, which ends the active generation): the format
                                           // kmb_gen_workspace_bytes sizes for, kmb_gen_begin packs in and kmb_gen_step hands to the blocks
  } gen;

  // ---- dropout sites.  ONE derivation for every site: the 16-bit threshold (rounded, capped), the seed drawn from the handle's seed and the
  // site's word, the keep scale.  A site's word is step * 0x10001 + its number; the numbers are
  //   hidden dropout (cfg.dropout, drop_site):  1, 2, 10 + 2 l, 11 + 2 l, 100 + 3 l .. 102 + 3 l
  //   attention dropout (attn_drop_site):       ATTN_SITE_BASE + 3 * layer + kind (0 encoder self, 1 decoder self, 2 decoder cross)
  //   activation dropout (act_drop_site):       ACT_SITE_BASE + 2 * layer + kind (0 encoder FFN, 1 decoder FFN)
  // No two words meet at any step, so adding a family moved no existing mask.  Attention numbers lie far above every hidden number and below the
  // next step's (a step advances the word by 0x10001).  ACT_SITE_BASE = 0x60000000 = 24576 * 0x10001 - 24576, so an activation site of step t
  // carries the word (t + 24576) * 0x10001 - 24576 + 2 l + k.  It equals a hidden site's word (t' * 0x10001 + c) only if 2 l + k - 24576 - c is a
  // multiple of 0x10001 = 65537, and an attention site's (c = 0x40000000 + 3 l' + k' = 16384 * 0x10001 - 16384 + 3 l' + k') only if
  // 2 l + k - 8192 - 3 l' - k' is: for layer counts below 4096 both differences lie strictly between -65537 and 0.
  //   classification-head dropout (cls_drop_site): CLS_SITE_BASE + 2 * head + which (head 0 mrm, 1 attribute, 2 relation; which 0 input, 1 hidden)
  // CLS_SITE_BASE = 0x50000000 = 20480 * 0x10001 - 20480, so a head site of step t carries the word (t + 20480) * 0x10001 - 20480 + s with
  // s = 2 head + which in 0 .. 5.  It equals a hidden site's word only if s - 20480 - c is a multiple of 65537 (c <= 102 + 3 l: the difference lies
  // strictly between -65537 and 0 while l < 14985), an attention site's only if s - 4096 - 3 l' - k' is (between -65537 and 0 while l' < 20479), and an
  // activation site's only if s + 4096 - 2 l'' - k'' is: that one is positive and at most 4101 while 2 l'' + k'' < 4096, and reaches 0 at layer 2048.
  // So no word of the family meets another at any step for layer counts below 2048 -- the bound of the four families together.
  // zero_off: a probability that rounds to threshold 0 is no dropout at all (seed 0 as well).  The two run-time families have it; drop_site never
  // had and keeps its seed there -- kmb_create does not validate cfg.dropout, so a probability below 2^-17 can reach it.
  KmbDrop site_drop(float p, uint64_t word, bool train, bool zero_off) const {
    KmbDrop dr{0u, 0u, 1.f};
    if (!train || p <= 0.f) return dr;
    uint32_t thr = (uint32_t)lrintf(p * 65536.f);
    if (thr > 65535u) thr = 65535u;
    if (zero_off && thr == 0u) return dr;
    dr.thr16 = thr;
    dr.seed = (uint32_t)kmbi::splitmix(seed ^ kmbi::splitmix(step * 0x10001ull + word));
    dr.scale = 1.f / (1.f - (float)thr / 65536.f);
    return dr;
  }
  KmbDrop drop_site(int site, bool train) const { return site_drop(cfg.dropout, (uint64_t)site, train, false); }
  // Attention dropout (F.dropout on the softmax weights, HF 3.0.2 SelfAttention): a run-time setting of the handle (kmb_set_attention_dropout), NOT
  // cfg.attention_dropout, which kmb_create keeps refusing.
  // attn_used[kind][layer]: what the LAST training forward launched with (zeros: none); backward reads it back instead of drawing again.
  static constexpr uint64_t ATTN_SITE_BASE = 0x40000000ull;
  float attn_p = 0.f;
  std::vector<KmbDrop> attn_used[3];
  KmbDrop attn_drop_site(int kind, int layer, bool train) {
    const KmbDrop dr = site_drop(attn_p, ATTN_SITE_BASE + (uint64_t)(3 * layer + kind), train, true);
    if (dr.thr16) attn_used[kind][layer] = dr;
    return dr;
  }
  KmbDrop attn_drop_used(int kind, int layer, bool train) const { return train ? attn_used[kind][layer] : KmbDrop{0u, 0u, 1.f}; }
  // Activation dropout (F.dropout on gelu(fc1(x)), HF 3.0.2 EncoderLayer / DecoderLayer): a run-time setting of the handle too
  // (kmb_set_activation_dropout; cfg.activation_dropout stays refused by kmb_create).  The fc1 launch folds the mask into its output AND the stored
  // GeLU' (KmbGemm, act 1 with drop_thr16), so backward neither stores nor redraws a mask.
  // act_used[kind][layer]: what the LAST training forward launched with (zeros: none), for kmb_activation_dropout_site.
  static constexpr uint64_t ACT_SITE_BASE = 0x60000000ull;
  float act_p = 0.f;
  std::vector<KmbDrop> act_used[2];
  KmbDrop act_drop_site(int kind, int layer, bool train) {
    const KmbDrop dr = site_drop(act_p, ACT_SITE_BASE + (uint64_t)(2 * layer + kind), train, true);
    if (dr.thr16) act_used[kind][layer] = dr;
    return dr;
  }
  // Classification-head dropout (the two F.dropout calls of HF 3.0.2 BartClassificationHead: on the head's input and on its tanh output): the third
  // run-time setting (kmb_set_classif_dropout; kmb_config does not carry it).  head_run masks the gathered input and a copy of the hidden
  // activations with the row kernel of heads.hip and hands the same KmbDrop to the two data-gradient GEMMs' epilogues, so backward redraws nothing.
  // cls_used[head][which]: what the LAST training forward launched with (zeros: none, or the head had no rows), for kmb_classif_dropout_site.
  static constexpr uint64_t CLS_SITE_BASE = 0x50000000ull;
  float cls_p = 0.f;
  // Label smoothing of the LM cross-entropy (kmb_set_label_smoothing): the fourth run-time setting; lm_head hands it to whichever head form runs.
  float label_smoothing = 0.f;
  int last_head_form = -1;   // 0 fp32, 1 bf16 two-kernel, 2 fused: the head the last forward with labels took (kmb_last_head_form)
  KmbDrop cls_used[3][2] = {{{0u, 0u, 1.f}, {0u, 0u, 1.f}}, {{0u, 0u, 1.f}, {0u, 0u, 1.f}}, {{0u, 0u, 1.f}, {0u, 0u, 1.f}}};
  KmbDrop cls_drop_site(int head, int which, bool train) {
    const KmbDrop dr = site_drop(cls_p, CLS_SITE_BASE + (uint64_t)(2 * head + which), train, true);
    if (dr.thr16) cls_used[head][which] = dr;
    return dr;
  }
  bf16_t* wb(size_t off) const { return kmbi::g_f32 ? reinterpret_cast<bf16_t*>(P + off) : PB + off; }   // GEMM B operand: bf16 mirror (fp32 master in validation mode)
  float* pf(size_t off) const { return P + off; }
  // Gradient accumulation (kmb_set_grad_accumulation): every gradient WRITER goes through gf() and lands in the stage, a second arena of
  // the caller's with this micro-batch's gradient only; kmb_backward folds each bucket of it into G in front of the bucket's completion
  // event (fold_bucket, engine_train.cpp).  Every READER (the optimizer, the norm, the exchange, the caller's views) uses G.
  float* GS = nullptr; size_t stage_floats = 0;
  bool accum = false;
  bool grad_fresh = true;   // kmb_zero_grad: the next backward's folds overwrite G; cleared by that backward
  float* gf(size_t off) const { return (accum ? GS : G) + off; }
};

namespace kmbi __attribute__((visibility("hidden"))) {

struct PrecisionScope {   // g_f32 follows the handle for the duration of one call
  explicit PrecisionScope(const kmb_handle* h) { g_f32 = h->fp32; }
  ~PrecisionScope() { g_f32 = false; g_small_slab = nullptr; g_small_floats = 0; }
};

struct AttnIO { const bf16_t* q; int ldq; const bf16_t* k; const bf16_t* v; int ldkv; int Tq, Tk; const int64_t* mask; int causal; };

// ---- engine.cpp
int check_bound(const kmb_handle* h);
KmbGemm gemm0();
int run_gemm(const KmbGemm& g, hipStream_t s);
KmbGemm lin_fwd(const bf16_t* x, int ldx, const bf16_t* w, const float* b, int M, int N, int K);                            // Y[M,N] = X[M,K] W[N,K]^T + b
KmbGemm lin_dgrad(const bf16_t* dy, int lddy, const bf16_t* w, int M, int N, int K);                                       // dX[M,K] = dY[M,N] W[N,K]
KmbGemm lin_wgrad(const bf16_t* dy, int lddy, const bf16_t* x, int ldx, float* dW, int M, int N, int K, float beta);       // dW[N,K] = dY[M,N]^T X[M,K]
int run_wgrad(kmb_handle* h, KmbGemm g, hipStream_t s, float* slab, size_t slab_floats);
int ensure_side(kmb_handle* h);
int order_behind(hipEvent_t e, hipStream_t from, hipStream_t to);
int order_behind(kmb_handle* h, hipStream_t from, hipStream_t to);
int wgrad_flush(kmb_handle* h, hipStream_t sA);
int wgrad_side(kmb_handle* h, const KmbGemm& g, hipStream_t sA);
hipStream_t reducer_stream(kmb_handle* h, hipStream_t sA);
int attn_forward(kmb_handle* h, const AttnIO& io, int B, int H, bf16_t* o, float* lse, KmbDrop adr, hipStream_t s);
int attn_backward(kmb_handle* h, const AttnIO& io, int B, int H, bf16_t* o, float* lse, const bf16_t* dO, bf16_t* dq, int lddq, bf16_t* dk,
                  bf16_t* dv, int lddkv, float* cs_q, float* cs_k, float* cs_v, int ld_cs, KmbDrop adr, hipStream_t s);
int ln_forward(const bf16_t* z, const float* gamma, const float* beta, bf16_t* y, float* mean, float* rstd, int M, int D, float eps, hipStream_t s);
int embed_ln_forward(const int64_t* ids, const int32_t* img_src, const float* E, const float* img_emb, const float* P, int pos_base, int S,
                     float scale, const float* gamma, const float* beta, bf16_t* z, bf16_t* y, float* mean, float* rstd, int M, int D, float eps,
                     KmbDrop drop, hipStream_t s);
extern int g_trace_layer;   // backward's current layer, for the KMB_BWD_TRACE table (kmb_debug_trace)
int trace(const char* name, const void* p, size_t bytes, hipStream_t s);
// ---- engine_train.cpp
int run_vocab_gemm(const KmbGemm& g, hipStream_t s, float* stats = nullptr, int* stats_blocks = nullptr);
int encoder_forward(kmb_handle* h, const EncoderBufs& eb, const kmb_batch& bt, bool train, hipStream_t s);

}  // namespace kmbi
