// Native data parallelism: the RCCL gradient exchange with its fused optimizer step, and the optimizer step on its own.
#include "engine_internal.h"

using namespace kmbi;

namespace {

#define NCCLCHK(expr)                                                                                          \
  do {                                                                                                         \
    ncclResult_t r_ = (expr);                                                                                  \
    if (r_ != ncclSuccess) return fail("%s failed: %s (%s:%d)", #expr, ncclGetErrorString(r_), __FILE__, __LINE__); \
  } while (0)

struct Piece { int bucket; size_t off, cnt; };

// the collectives of one gradient exchange: every bucket (backward completion order) cut into pieces of at most `cap`
// elements whose boundaries stay 64-element aligned (the fused optimizer's and the shards' alignment)
std::vector<Piece> comm_pieces(const kmb_handle* h, int64_t max_piece_elems) {
  const size_t cap = max_piece_elems > 0 ? (size_t)max_piece_elems : (size_t)16 << 20;
  std::vector<Piece> out;
  for (size_t i = 0; i < h->buckets.size(); ++i) {
    const size_t off = h->buckets[i].off, cnt = h->buckets[i].count;
    if (cnt == 0) continue;
    if (cnt > cap) {
      const size_t n = (cnt + cap - 1) / cap;
      const size_t step = align_up((cnt + n - 1) / n, 64);
      for (size_t s0 = 0; s0 < cnt; s0 += step) out.push_back({(int)i, off + s0, std::min(step, cnt - s0)});
    } else {
      out.push_back({(int)i, off, cnt});
    }
  }
  return out;
}

// piece i of the exchange as rank `rank` of `world` sees it: a pure function of the arena layout (no communicator, no device).
// Every collective of kmb_allreduce_grads / kmb_comm_gather_moments takes its offsets from here, so the world > 1 arithmetic
// is testable on a CPU (tests/test_comm_plan_cpu.py).
int comm_plan_piece(const kmb_handle* h, const Piece& pc, int world, int rank, kmb_comm_piece* out) {
  const size_t W = (size_t)world;
  out->bucket = pc.bucket; out->offset = (int64_t)pc.off; out->count = (int64_t)pc.cnt;
  const size_t shard = pc.cnt / W;   // pieces are multiples of 64 elements and world divides 8: shards stay 8-element aligned
  out->shard = (shard * W == pc.cnt && (shard & 7) == 0) ? (int64_t)shard : 0;   // 0: this piece has no aligned shards (algo 1 refuses it)
  out->mine = (int64_t)(pc.off + (size_t)rank * shard);
  const size_t iw0 = h->img_w, iw1 = h->img_w + (size_t)h->d * h->Fin;
  out->repad_piece = (pc.off < iw1 && pc.off + pc.cnt > iw0) ? 1 : 0;
  out->repad_shard = ((size_t)out->mine < iw1 && (size_t)out->mine + shard > iw0) ? 1 : 0;
  return 0;
}

int comm_ready(const kmb_handle* h, const char* who) {
  if (!h->comm || !h->comm_stream) return fail("%s: no communicator (call kmb_comm_init first)", who);
  if (!h->P || !h->G) return fail("%s: arenas are not bound", who);
  return 0;
}

// the optimizer update of arena range [off, off + cnt) on stream s (kmb_adamw_step and the fused step of the exchange); the padded
// image-weight mirror lives outside the flat mirror
// state: the device record of a clipped / guarded step (kmb_adamw_step_dev), null for the host-state step
int adamw_range(kmb_handle* h, const KmbAdamW& hp, size_t off, size_t cnt, hipStream_t s, const KmbStepState* state = nullptr) {
  if (!h->M1 || !h->M2) return fail("fused optimizer step: the moment arenas are not bound");
  if (state) HIPCHK(kmb_adamw_dev_launch(h->P + off, h->G + off, h->M1 + off, h->M2 + off, h->PB + off, cnt, hp, state, s));
  else HIPCHK(kmb_adamw_launch(h->P + off, h->G + off, h->M1 + off, h->M2 + off, h->PB + off, cnt, hp, s));
  h->mirror_version++;
  const size_t iw0 = h->img_w, iw1 = h->img_w + (size_t)h->d * h->Fin;
  if (off < iw1 && off + cnt > iw0)
    HIPCHK(kmb_cast_rows_launch(h->pf(h->img_w), h->Fin, h->imgw_pad, h->Fpad, h->d, h->Fin, s));
  return 0;
}

// ---- clipped / guarded step (include/kmbart.h).  Partial slots: a piece of n elements takes kmb_grad_sumsq_slots(n); the buffer holds enough for
// any cut of the arena into parameter runs x buckets (a run of parameters needs at most the sum of its parameters' slots plus one per parameter for
// the alignment gap in front of it; a bucket boundary adds at most one piece).
constexpr size_t STEP_PARTIALS_AT = 64;   // byte offset of the partial sums behind the record
int step_slots_cap(const kmb_handle* h) {
  size_t n = h->buckets.size();
  for (const auto& p : h->params) n += (size_t)kmb_grad_sumsq_slots((size_t)p.rows * p.cols) + 1;
  return (int)n;
}
int step_ready(const kmb_handle* h, const char* who) {
  if (!h->step_state) return fail("%s: no step-state buffer (call kmb_bind_step_state first)", who);
  if (!h->P || !h->G || !h->M1 || !h->M2) return fail("%s: arenas are not bound", who);
  const char *a = (const char*)h->step_state, *b = (const char*)(h->step_partials + h->step_slots);
  if (h->ws && a < h->ws + h->ws_bytes && b > h->ws) return fail("%s: the step-state buffer lies inside the workspace", who);
  return 0;
}
}  // namespace

extern "C" {

int kmb_adamw_step(kmb_handle* h, const KmbAdamW* hp, int64_t offset, int64_t count, void* stream) {
  if (!h->P || !h->G || !h->M1 || !h->M2) return fail("kmb_adamw_step: arenas are not bound");
  if (offset < 0 || count < 0 || (size_t)(offset + count) > h->arena) return fail("kmb_adamw_step: range out of the arena");
  if (offset & 7) return fail("kmb_adamw_step: offset must be a multiple of 8 elements");
  return adamw_range(h, *hp, (size_t)offset, (size_t)count, (hipStream_t)stream);
}

// ---- clipped / guarded step
int64_t kmb_step_state_bytes(const kmb_handle* h) { return (int64_t)(STEP_PARTIALS_AT + sizeof(double) * (size_t)step_slots_cap(h)); }

int kmb_bind_step_state(kmb_handle* h, void* buf, int64_t bytes) {
  static_assert(sizeof(KmbStepState) == 24 && sizeof(KmbStepState) <= STEP_PARTIALS_AT, "KmbStepState is six 4-byte fields");
  if (!buf || bytes < kmb_step_state_bytes(h)) return fail("kmb_bind_step_state: the buffer is smaller than kmb_step_state_bytes");
  if ((uintptr_t)buf & 15) return fail("kmb_bind_step_state: the buffer must be 16-byte aligned");
  if (h->ws && (char*)buf < h->ws + h->ws_bytes && (char*)buf + bytes > h->ws) return fail("kmb_bind_step_state: the buffer lies inside the workspace");
  HIPCHK(hipMemset(buf, 0, (size_t)kmb_step_state_bytes(h)));
  h->step_state = (KmbStepState*)buf;
  h->step_partials = (double*)((char*)buf + STEP_PARTIALS_AT);
  h->step_slots = step_slots_cap(h);
  return 0;
}

int kmb_grad_sumsq(kmb_handle* h, int64_t offset, int64_t count, float grad_scale, int32_t slot0, void* stream) {
  KCHK(step_ready(h, "kmb_grad_sumsq"));
  if (offset < 0 || count < 0 || (size_t)(offset + count) > h->arena) return fail("kmb_grad_sumsq: range out of the arena");
  if (offset & 3) return fail("kmb_grad_sumsq: offset must be a multiple of 4 elements");
  if (slot0 < 0 || slot0 + (count > 0 ? kmb_grad_sumsq_slots((size_t)count) : 0) > h->step_slots) return fail("kmb_grad_sumsq: slots out of the step-state buffer");
  HIPCHK(kmb_grad_sumsq_launch(h->G + offset, (size_t)count, grad_scale, h->step_partials + slot0, (hipStream_t)stream));
  return 0;
}

int kmb_clip_finish(kmb_handle* h, const KmbAdamW* hp, float max_norm, int32_t skip_nonfinite, int32_t nslots, void* stream) {
  KCHK(step_ready(h, "kmb_clip_finish"));
  if (!hp) return fail("kmb_clip_finish: hp is required");
  if (nslots <= 0 || nslots > h->step_slots) return fail("kmb_clip_finish: nslots out of the step-state buffer");
  HIPCHK(kmb_clip_finish_launch(h->step_partials, nslots, max_norm, skip_nonfinite, *hp, h->step_state, (hipStream_t)stream));
  return 0;
}

int kmb_adamw_step_dev(kmb_handle* h, const KmbAdamW* hp, int64_t offset, int64_t count, void* stream) {
  KCHK(step_ready(h, "kmb_adamw_step_dev"));
  if (!hp) return fail("kmb_adamw_step_dev: hp is required");
  if (offset < 0 || count < 0 || (size_t)(offset + count) > h->arena) return fail("kmb_adamw_step_dev: range out of the arena");
  if (offset & 7) return fail("kmb_adamw_step_dev: offset must be a multiple of 8 elements");
  return adamw_range(h, *hp, (size_t)offset, (size_t)count, (hipStream_t)stream, h->step_state);
}

int kmb_step_state_read(kmb_handle* h, KmbStepState* host_record, void* stream) {
  if (!h->step_state) return fail("kmb_step_state_read: no step-state buffer (call kmb_bind_step_state first)");
  if (!host_record) return fail("kmb_step_state_read: host_record is required");
  HIPCHK(hipMemcpyAsync(host_record, h->step_state, sizeof(KmbStepState), hipMemcpyDeviceToHost, (hipStream_t)stream));
  return 0;
}

int kmb_step_state_set_steps(kmb_handle* h, int32_t steps, void* stream) {
  if (!h->step_state) return fail("kmb_step_state_set_steps: no step-state buffer (call kmb_bind_step_state first)");
  if (steps < 0) return fail("kmb_step_state_set_steps: steps must not be negative");
  HIPCHK(hipMemsetD32Async((hipDeviceptr_t)&h->step_state->steps, steps, 1, (hipStream_t)stream));
  return 0;
}

int kmb_comm_unique_id(void* id_host) {
  static_assert(sizeof(ncclUniqueId) == KMB_COMM_ID_BYTES, "ncclUniqueId is 128 bytes");
  if (!id_host) return fail("kmb_comm_unique_id: id_host is required");
  ncclUniqueId id;
  NCCLCHK(ncclGetUniqueId(&id));
  memcpy(id_host, &id, sizeof(id));
  return 0;
}

int kmb_comm_init(kmb_handle* h, int rank, int world, const void* id_host) {
  if (!id_host || world < 1 || rank < 0 || rank >= world) return fail("kmb_comm_init: bad rank / world / id");
  if (h->comm) return fail("kmb_comm_init: this handle already has a communicator");
  ncclUniqueId id;
  memcpy(&id, id_host, sizeof(id));
  NCCLCHK(ncclCommInitRank(&h->comm, world, id, rank));
  h->comm_rank = rank; h->comm_world = world;
  HIPCHK(hipStreamCreateWithFlags(&h->comm_stream, hipStreamNonBlocking));
  HIPCHK(hipEventCreateWithFlags(&h->comm_ev, hipEventDisableTiming));
  return 0;
}

int kmb_comm_destroy(kmb_handle* h) {
  if (h->comm) { (void)ncclCommDestroy(h->comm); h->comm = nullptr; }
  if (h->comm_stream) { (void)hipStreamDestroy(h->comm_stream); h->comm_stream = nullptr; }
  if (h->comm_ev) { (void)hipEventDestroy(h->comm_ev); h->comm_ev = nullptr; }
  h->comm_world = 0; h->comm_rank = 0;
  //  without a communicator nothing can gather the moment shards any more: the flag must not outlive it, or a later plain
  // AdamW.step() / state_dict() would ask for a collective on a destroyed communicator.  The Python wrapper gathers BEFORE it destroys
  // (kmbart/engine.py::comm_destroy); a caller of the C-ABI that destroys with sharded moments keeps this rank's shard only.
  h->moments_sharded = false;
  return 0;
}

int kmb_comm_info(const kmb_handle* h, int32_t* rank, int32_t* world) {
  if (rank) *rank = h->comm_rank;
  if (world) *world = h->comm ? h->comm_world : 0;
  return 0;
}

int kmb_comm_broadcast_params(kmb_handle* h, int root, void* stream) {
  hipStream_t s = (hipStream_t)stream;
  KCHK(comm_ready(h, "kmb_comm_broadcast_params"));
  if (root < 0 || root >= h->comm_world) return fail("kmb_comm_broadcast_params: root out of range");
  NCCLCHK(ncclBroadcast(h->P, h->P, h->arena, ncclFloat, root, h->comm, s));
  NCCLCHK(ncclBroadcast(h->flb, h->flb, (size_t)h->V, ncclFloat, root, h->comm, s));
  return kmb_sync_params(h, stream);
}

int64_t kmb_comm_pieces(const kmb_handle* h, int64_t max_piece_elems) { return (int64_t)comm_pieces(h, max_piece_elems).size(); }

int kmb_comm_plan(const kmb_handle* h, int world, int rank, int64_t max_piece_elems, int64_t i, kmb_comm_piece* out) {
  if (!h || !out) return fail("kmb_comm_plan: null argument");
  if (world < 1 || rank < 0 || rank >= world) return fail("kmb_comm_plan: bad rank %d / world %d", rank, world);
  const std::vector<Piece> pcs = comm_pieces(h, max_piece_elems);
  if (i < 0 || i >= (int64_t)pcs.size()) return fail("kmb_comm_plan: piece %lld out of range (%zu pieces)", (long long)i, pcs.size());
  return comm_plan_piece(h, pcs[(size_t)i], world, rank, out);
}
int kmb_comm_moments_sharded(const kmb_handle* h) { return h && h->moments_sharded ? 1 : 0; }

int kmb_allreduce_grads(kmb_handle* h, const kmb_allreduce_opts* opts, void* compute_stream) {
  KCHK(comm_ready(h, "kmb_allreduce_grads"));
  static const kmb_allreduce_opts dflt{0, 0, 0, nullptr};
  const kmb_allreduce_opts& o = opts ? *opts : dflt;
  const int W = h->comm_world, rank = h->comm_rank;
  if (o.algo != 0 && o.algo != 1) return fail("kmb_allreduce_grads: algo must be 0 (all-reduce) or 1 (reduce-scatter + all-gather)");
  if (o.algo == 1 && (8 % W) != 0) return fail("kmb_allreduce_grads: algo 1 needs a world size that divides 8 (got %d)", W);
  if (o.algo == 1) h->comm_piece_cap = o.max_piece_elems;
  hipStream_t cs = h->comm_stream;
  if (o.after_compute) {
    KCHK(order_behind(h->comm_ev, (hipStream_t)compute_stream, cs));   // (its own event: the ring exists only once a backward has run)
  }
  int waited = -1;
  for (const Piece& pc : comm_pieces(h, o.max_piece_elems)) {
    if (pc.bucket != waited) {   // the bucket's gradients are complete (both compute streams are past it: kmb_backward)
      if (!h->events[pc.bucket]) return fail("kmb_allreduce_grads: bucket %d has no completion event (run kmb_backward first)", pc.bucket);
      HIPCHK(hipStreamWaitEvent(cs, h->events[pc.bucket], 0));
      waited = pc.bucket;
    }
    float* g = h->G + pc.off;
    if (o.algo == 0) {
      NCCLCHK(ncclAllReduce(g, g, pc.cnt, ncclFloat, ncclAvg, h->comm, cs));
      if (o.adamw) KCHK(adamw_range(h, *o.adamw, pc.off, pc.cnt, cs));
      continue;
    }
    // reduce-scatter: rank r ends up with the mean of shard r (in place: recvbuff = sendbuff + r * shard)
    kmb_comm_piece pl;
    KCHK(comm_plan_piece(h, pc, W, rank, &pl));
    if (pl.shard == 0) return fail("kmb_allreduce_grads: piece of %zu elements does not split into %d aligned shards", pc.cnt, W);
    const size_t shard = (size_t)pl.shard, mine = (size_t)pl.mine;
    NCCLCHK(ncclReduceScatter(g, h->G + mine, shard, ncclFloat, ncclAvg, h->comm, cs));
    if (o.adamw) {
      KCHK(adamw_range(h, *o.adamw, mine, shard, cs));                                              // 30 B / parameter / W
      NCCLCHK(ncclAllGather(h->P + mine, h->P + pc.off, shard, ncclFloat, h->comm, cs));           // updated fp32 masters
      if (W > 1) {   // the other ranks' shards of the bf16 mirror (this rank's was written by the optimizer kernel)
        HIPCHK(kmb_cast_f32_bf16_launch(h->P + pc.off, h->PB + pc.off, pc.cnt, cs));
        h->mirror_version++;
        if (pl.repad_piece)
          HIPCHK(kmb_cast_rows_launch(h->pf(h->img_w), h->Fin, h->imgw_pad, h->Fpad, h->d, h->Fin, cs));
        h->moments_sharded = true;   // exp_avg / exp_avg_sq are current on the owning rank's shard only
      }
    } else {
      NCCLCHK(ncclAllGather(h->G + mine, g, shard, ncclFloat, h->comm, cs));
    }
  }
  return 0;
}

int kmb_comm_wait(kmb_handle* h, void* compute_stream) {
  if (!h->comm_stream) return fail("kmb_comm_wait: no communicator");
  return order_behind(h->comm_ev, h->comm_stream, (hipStream_t)compute_stream);
}

int kmb_comm_gather_moments(kmb_handle* h, void* compute_stream) {
  KCHK(comm_ready(h, "kmb_comm_gather_moments"));
  if (!h->M1 || !h->M2) return fail("kmb_comm_gather_moments: the moment arenas are not bound");
  const int W = h->comm_world, rank = h->comm_rank;
  if ((8 % W) != 0) return fail("kmb_comm_gather_moments: world size must divide 8");
  hipStream_t s = (hipStream_t)compute_stream;
  for (const Piece& pc : comm_pieces(h, h->comm_piece_cap)) {
    kmb_comm_piece pl;
    KCHK(comm_plan_piece(h, pc, W, rank, &pl));
    if (pl.shard == 0) return fail("kmb_comm_gather_moments: piece of %zu elements does not split into %d aligned shards", pc.cnt, W);
    NCCLCHK(ncclAllGather(h->M1 + pl.mine, h->M1 + pc.off, (size_t)pl.shard, ncclFloat, h->comm, s));
    NCCLCHK(ncclAllGather(h->M2 + pl.mine, h->M2 + pc.off, (size_t)pl.shard, ncclFloat, h->comm, s));
  }
  h->moments_sharded = false;
  return 0;
}

}  // extern "C"
