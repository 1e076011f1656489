"""Python host of libkmbart_hip.so: owns the device arenas (torch tensors) and forwards calls
through the C-ABI.  torch is used for memory, streams and torch.distributed only."""
import ctypes as C
import os

import torch

from . import _lib
from ._lib import KmbAdamW, KmbBatch, KmbConfig, KmbForwardOpts, KmbPretrain, check, ptr

_CFG_INT_FIELDS = ("vocab_size", "d_model", "encoder_layers", "decoder_layers", "encoder_attention_heads",
                   "decoder_attention_heads", "encoder_ffn_dim", "decoder_ffn_dim", "max_position_embeddings",
                   "extra_pos_embeddings", "image_feature_size", "pad_token_id", "bos_token_id", "eos_token_id",
                   "img_feat_id", "cls_token_id")


LOSS_REDUCTIONS = {"mean": 0, "sum": 1}   # kmb_forward_opts.loss_reduction


def check_targets_per_input(targets_per_input, input_ids, **decoder_side):
    """The ONE check of `targets_per_input` (Engine.forward and the model classes call it): None and 1 mean one target per input and return 1;
    anything below 1 is a ValueError; G > 1: every given decoder-side tensor (by keyword: its name goes into the message) must have exactly G
    rows per input, row i belonging to input i // G.  Pure shape arithmetic -- no device, no engine."""
    if targets_per_input is None:
        return 1
    G = int(targets_per_input)
    if G < 1:
        raise ValueError("targets_per_input must be a positive integer, got %r" % (targets_per_input,))
    if G == 1:
        return 1
    B = int(input_ids.shape[0])
    for name, t in decoder_side.items():
        if t is not None and int(t.shape[0]) != B * G:
            raise ValueError("targets_per_input = %d: %s needs %d x %d = %d rows (row i belongs to input i // %d), got %d"
                             % (G, name, G, B, B * G, G, int(t.shape[0])))
    return G


def _stream():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def pack_features(image_features, feat_dim, device):
    """list[B] of [R_i, F] fp32 (R_i may be 0 -> torch.empty(0), collation.py:73-76)
    -> (packed [Ntot, F] fp32 on device, offsets int32 [B+1] on device, Ntot)."""
    if hasattr(image_features, "packed") and hasattr(image_features, "offsets"):   # kmbart.data.PackedFeatures
        return (image_features.packed.to(device=device, dtype=torch.float32).contiguous(),
                image_features.offsets.to(device=device, dtype=torch.int32).contiguous(), image_features.n_total)
    lens = [int(x.shape[0]) if x.dim() == 2 else 0 for x in image_features]
    offs = [0]
    for n in lens:
        offs.append(offs[-1] + n)
    non_empty = [x.to(device=device, dtype=torch.float32) for x, n in zip(image_features, lens) if n > 0]
    for x in non_empty:
        if x.shape[1] != feat_dim:
            raise ValueError("image feature width %d != config.image_feature_size %d" % (x.shape[1], feat_dim))
    if not non_empty:
        packed = torch.zeros((1, feat_dim), device=device)
    elif len(non_empty) == 1:
        packed = non_empty[0].contiguous()
    elif torch.device(device).type != "cuda":
        packed = torch.cat(non_empty, 0).contiguous()   # host-side use (tests of the batch layout): no kernel to launch
    else:
        # ONE launch per 128 tensors (kmb_pack_features) instead of torch.cat, which on this stack is a batched kernel plus ~one blit
        # per tensor (70 copy launches in front of a 64-sample generate); the sources are kept alive by the caller's `keep` list
        srcs = [x.contiguous() for x in non_empty]
        packed = torch.empty((offs[-1], feat_dim), dtype=torch.float32, device=device)
        ptrs = (C.c_void_p * len(srcs))(*[x.data_ptr() for x in srcs])
        rows = (C.c_int32 * len(srcs))(*[int(x.shape[0]) for x in srcs])
        with torch.cuda.device(device):
            check(_lib.load().kmb_pack_features(ptrs, rows, len(srcs), int(feat_dim), ptr(packed), _stream()))
        packed._kmb_sources = srcs   # the kernel reads them in stream order: alive as long as the packed buffer is
    offsets = torch.tensor(offs, dtype=torch.int32).to(device)
    return packed, offsets, offs[-1]


def refuse_ignored_head_labels(head, labels):
    """The attribute and relation heads take class ids only.  The reference's collator builds their labels from the dataset's
    attribute_ids / predicate_id (src/data/collation.py:149-190) and never writes -100 there -- only the LM labels are masked
    (:192-195) -- so an ignored label cannot reach these heads on the reference's data path.  The engine's head loss divides by the
    number of rows while its gradient divides by the number of valid labels (csrc/engine_train.cpp head_run): with a -100 the two would
    disagree with each other and with CrossEntropyLoss().  Refused here instead of being averaged one way or the other."""
    if labels is None or labels.numel() == 0:
        return
    if bool((labels == -100).any()):
        raise ValueError("%s labels hold -100: the %s head takes class ids only (the reference's collator never emits an ignored "
                         "label for it); drop those rows from the head's row list instead" % (head, head))


class StepRecord:
    """A device copy of a KmbStepState (Engine.step_record)."""

    def __init__(self, dev):
        self.dev = dev

    @staticmethod
    def decode(host_bytes):
        r = _lib.KmbStepState.from_buffer_copy(host_bytes.numpy().tobytes())
        return {"norm": float(r.norm), "coef": float(r.coef), "step_size": float(r.step_size), "applied": int(r.applied),
                "steps": int(r.steps), "skipped": int(r.skipped)}

    def read(self):
        return self.decode(self.dev.cpu())


class Engine:
    """One model replica on one GPU."""

    def __init__(self, config, device, with_heads=False):
        self.lib = _lib.load()
        if not torch.cuda.is_available():
            raise _lib.KmbError("the KM-BART hot path needs an MI355X (HIP) device; there is no CPU fallback")
        self.device = torch.device(device)
        if self.device.type != "cuda":
            raise _lib.KmbError("Engine device must be a HIP device ('cuda:N'), got %s" % device)
        self.config = config
        c = KmbConfig()
        for f in _CFG_INT_FIELDS:
            setattr(c, f, int(getattr(config, f)))
        c.scale_embedding = 1 if getattr(config, "scale_embedding", False) else 0
        c.dropout = float(config.dropout)
        c.attention_dropout = 0.0   # a run-time setting of the handle (set_attention_dropout below); the creation struct refuses it
        c.activation_dropout = 0.0   # likewise (set_activation_dropout)
        c.layer_norm_eps = 1e-5
        if with_heads:  # MultiModalBartForPreTraining (reference src/model/model.py:133-158)
            c.num_labels = int(config.num_labels)
            c.num_attributes = int(config.num_attributes)
            c.num_relations = int(config.num_relations)
        self._ccfg = c
        h = C.c_void_p()
        check(self.lib.kmb_create(C.byref(c), C.byref(h)))
        self.h = h
        self.set_attention_dropout(float(getattr(config, "attention_dropout", 0.0)))
        self.set_activation_dropout(float(getattr(config, "activation_dropout", 0.0)))
        self.set_classif_dropout(float(getattr(config, "classif_dropout", 0.0)))   # (without heads there is nothing to drop: no effect)
        self.set_label_smoothing(float(getattr(config, "label_smoothing", 0.0)))
        with torch.cuda.device(self.device):
            n = self.lib.kmb_arena_elems(h)
            nb = self.lib.kmb_bf16_arena_elems(h)
            self.n = n
            self.params = torch.zeros(n, dtype=torch.float32, device=self.device)
            self.grads = torch.zeros(n, dtype=torch.float32, device=self.device)
            self.exp_avg = torch.zeros(n, dtype=torch.float32, device=self.device)
            self.exp_avg_sq = torch.zeros(n, dtype=torch.float32, device=self.device)
            self.params_bf16 = torch.zeros(nb, dtype=torch.bfloat16, device=self.device)
            self.final_logits_bias = torch.zeros(int(config.vocab_size), dtype=torch.float32, device=self.device)
            check(self.lib.kmb_bind_arenas(h, ptr(self.params), ptr(self.grads), ptr(self.exp_avg),
                                           ptr(self.exp_avg_sq), ptr(self.params_bf16), ptr(self.final_logits_bias)))
        self.index = {}  # name -> (offset, rows, cols)
        name, off, rows, cols = C.c_char_p(), C.c_int64(), C.c_int32(), C.c_int32()
        for i in range(self.lib.kmb_param_count(h)):
            check(self.lib.kmb_param_info(h, i, C.byref(name), C.byref(off), C.byref(rows), C.byref(cols)))
            self.index[name.value.decode()] = (off.value, rows.value, cols.value)
        self.logits_ld = self.lib.kmb_logits_ld(h)
        self.workspace = None
        self._loss = torch.zeros(1, dtype=torch.float32, device=self.device)
        self._keep = []  # tensors the in-flight kernels read
        self.step_count = 0
        self.fwd_serial = 0      # bumped by every call that rewrites the workspace (LazyLogits validity)
        self.gen_logits_bytes = 4   # bytes per element of the decode step's logits buffer
        self.fp32_mode = False
        self.gen_weight_format = "bf16"

    def __del__(self):
        try:
            if getattr(self, "h", None):
                self.lib.kmb_destroy(self.h)
                self.h = None
        except Exception:
            pass

    # ---- parameters -------------------------------------------------------------------------
    def view(self, arena, name):
        off, rows, cols = self.index[name]
        t = arena[off: off + rows * cols]
        return t.view(cols) if rows == 1 else t.view(rows, cols)

    def sync_params(self):
        """fp32 master -> bf16 mirror (after init / load_state_dict / manual edits)."""
        with torch.cuda.device(self.device):
            check(self.lib.kmb_sync_params(self.h, _stream()))

    def set_precision(self, fp32):
        """fp32 validation mode (True) / bf16 product mode (False).  Mode True runs the eval-mode forward with float
        activations on exact-fp32 kernels against the fp32 master weights (parity evidence, never the measured path);
        encoder states then come back as float32 tensors."""
        torch.cuda.synchronize(self.device)
        check(self.lib.kmb_set_precision(self.h, 1 if fp32 else 0))
        self.fp32_mode = bool(fp32)
        self.workspace = None
        self.fwd_serial += 1

    @property
    def act_dtype(self):
        return torch.float32 if self.fp32_mode else torch.bfloat16

    def set_seed(self, seed):
        check(self.lib.kmb_set_seed(self.h, C.c_uint64(int(seed) & (2 ** 64 - 1))))

    def set_attention_dropout(self, p):
        """Dropout probability of the attention weights (config.attention_dropout), from the next training-mode forward on;
        eval forwards, score() and generation never drop."""
        check(self.lib.kmb_set_attention_dropout(self.h, C.c_float(float(p))))
        self.attention_dropout = float(p)

    def attention_dropout_site(self, kind, layer):
        """(thr16, seed) the last training forward used at an attention site (kind 0 encoder self, 1 decoder self, 2 decoder
        cross); (0, 0) when it ran without dropout.  kmb_op_dropout_mask(seed, thr16 / 65536, B * H * Tq, Tk) rebuilds the mask."""
        thr, seed = C.c_uint32(0), C.c_uint32(0)
        check(self.lib.kmb_attention_dropout_site(self.h, int(kind), int(layer), C.byref(thr), C.byref(seed)))
        return int(thr.value), int(seed.value)

    def set_activation_dropout(self, p):
        """Dropout probability of the FFN's hidden activations (config.activation_dropout), from the next training-mode forward
        on; eval forwards, score() and generation never drop."""
        check(self.lib.kmb_set_activation_dropout(self.h, C.c_float(float(p))))
        self.activation_dropout = float(p)

    def activation_dropout_site(self, kind, layer):
        """(thr16, seed) the last training forward used at an FFN site (kind 0 encoder, 1 decoder); (0, 0) when it ran without
        dropout.  kmb_op_dropout_mask(seed, thr16 / 65536, rows, F) rebuilds the mask (rows = B * S encoder, B * T decoder)."""
        thr, seed = C.c_uint32(0), C.c_uint32(0)
        check(self.lib.kmb_activation_dropout_site(self.h, int(kind), int(layer), C.byref(thr), C.byref(seed)))
        return int(thr.value), int(seed.value)

    def set_classif_dropout(self, p):
        """Dropout probability of the classification heads (config.classif_dropout: a head's input and its tanh output), from the
        next training-mode pre-training forward on; eval forwards, score() and generation never drop."""
        check(self.lib.kmb_set_classif_dropout(self.h, C.c_float(float(p))))
        self.classif_dropout = float(p)

    def set_label_smoothing(self, eps):
        """Label smoothing of the LM cross-entropy (torch's CrossEntropyLoss(label_smoothing=eps)), 0 <= eps < 1, from the next forward
        with labels on, in train and eval mode alike; score() and generation are untouched.  0 runs exactly what ran without it."""
        check(self.lib.kmb_set_label_smoothing(self.h, C.c_float(float(eps))))
        self.label_smoothing = float(eps)

    def last_head_form(self):
        """Which LM head the last forward with labels took: 0 fp32 logits, 1 bf16 logits turned into their gradient in place, 2 the fused
        head (no pass over the logits); -1 before the first."""
        return int(self.lib.kmb_last_head_form(self.h))

    def classif_dropout_site(self, head, which):
        """(thr16, seed) the last training forward used at a head site (head 0 masked-region, 1 attribute, 2 relation; which 0 the
        head's input, 1 its hidden activations); (0, 0) when it ran without dropout, the head had no rows or does not exist.
        kmb_op_dropout_mask(seed, thr16 / 65536, n, d_in or d_model) rebuilds the mask over the head's n gathered rows."""
        thr, seed = C.c_uint32(0), C.c_uint32(0)
        check(self.lib.kmb_classif_dropout_site(self.h, int(head), int(which), C.byref(thr), C.byref(seed)))
        return int(thr.value), int(seed.value)

    # ---- workspace --------------------------------------------------------------------------
    def _ensure_ws(self, nbytes):
        if self.workspace is None or self.workspace.numel() < nbytes:
            torch.cuda.synchronize(self.device)
            self.workspace = None
            self.workspace = torch.empty(int(nbytes) + 256, dtype=torch.uint8, device=self.device)
            check(self.lib.kmb_bind_workspace(self.h, ptr(self.workspace), self.workspace.numel()))
            self._poison()

    def _poison(self):
        """KMB_POISON=1 (diagnostic, tests/conftest.py --poison): every byte of the workspace becomes 0xFF -- a NaN in
        bf16 and in fp32, -1 in the integer tables -- when it is allocated and before every forward / generate, so a
        kernel that reads activation, scratch or slab memory nobody wrote in THIS call returns NaN deterministically
        instead of whatever the allocator's block happened to hold.  (torch.empty is the product behaviour.)"""
        if self.workspace is not None and os.environ.get("KMB_POISON") == "1":
            self.workspace.fill_(0xFF)
            # (re-binding tells the library that nothing it left in the workspace -- e.g. the packed decoder weights of the last
            #  generate -- is there any more)
            check(self.lib.kmb_bind_workspace(self.h, ptr(self.workspace), self.workspace.numel()))

    def _batch(self, input_ids, image_features, attention_mask, decoder_input_ids, decoder_attention_mask, labels):
        dev = self.device

        def i64(t):
            return None if t is None else t.to(device=dev, dtype=torch.int64).contiguous()

        input_ids = i64(input_ids)
        B, S = input_ids.shape
        packed, offsets, ntot = pack_features(image_features, int(self.config.image_feature_size), dev)
        attention_mask = i64(attention_mask)
        decoder_input_ids = i64(decoder_input_ids)
        decoder_attention_mask = i64(decoder_attention_mask)
        labels = i64(labels)
        T = decoder_input_ids.shape[1] if decoder_input_ids is not None else 1
        b = KmbBatch(B=B, S=S, T=T, input_ids=ptr(input_ids), attention_mask=ptr(attention_mask),
                     image_features=ptr(packed), feat_offsets=ptr(offsets), n_features=ntot,
                     decoder_input_ids=ptr(decoder_input_ids), decoder_attention_mask=ptr(decoder_attention_mask),
                     labels=ptr(labels))
        keep = [input_ids, packed, offsets, attention_mask, decoder_input_ids, decoder_attention_mask, labels]
        return b, keep, (B, S, T, ntot)

    def _loss_opts(self, opts, keep, loss_weights, loss_reduction, labels, B, T):
        """Fills kmb_forward_opts.row_weights / loss_reduction: [B] weights are broadcast over T, the result is a contiguous float32
        [B, T] on the device that `keep` holds until the forward is enqueued.  Device ops only."""
        if loss_reduction not in LOSS_REDUCTIONS:
            raise ValueError("loss_reduction must be 'mean' or 'sum', got %r" % (loss_reduction,))
        opts.loss_reduction = LOSS_REDUCTIONS[loss_reduction]
        if loss_weights is None:
            return
        if labels is None:
            raise ValueError("loss_weights weigh the rows' cross-entropy: they need labels")
        w = loss_weights.detach().to(device=self.device, dtype=torch.float32)
        if tuple(w.shape) == (B,):
            w = w.unsqueeze(1).expand(B, T)
        elif tuple(w.shape) != (B, T):
            raise ValueError("loss_weights must be [batch] or [batch, tgt_len] = %s, got %s" % ((B, T), tuple(loss_weights.shape)))
        w = w.contiguous()
        opts.row_weights = ptr(w)
        keep.append(w)

    # ---- training step ----------------------------------------------------------------------
    def forward(self, input_ids, image_features, attention_mask=None, decoder_input_ids=None,
                decoder_attention_mask=None, labels=None, train=False, need_grad=False, want_logits=False,
                want_encoder=True, encoder_states=None, want_decoder_states=False, skip_head=False,
                loss_weights=None, loss_reduction="mean", targets_per_input=None):
        """Returns (loss [1] or None, logits [B,T,V] fp32 or None, encoder_out [B,S,D] or None); with
        want_decoder_states a 4th element, the last decoder hidden states [B,T,D].  `encoder_states` [B,S,D] skips the
        encoder (reference src/model/model.py:76-83); activations are bf16 (float32 in the fp32 validation mode).
        `loss_weights` ([B, T] per decoder row or [B] per sequence, indexed like `labels`) and `loss_reduction` ("mean" / "sum"):
        kmb_forward_opts.row_weights / loss_reduction.
        `targets_per_input` = G > 1 (kmb_forward_opts.targets_per_input): the decoder tensors, `labels` and `loss_weights` have B * G rows,
        row i belonging to input i // G; the encoder side runs once on the B inputs; logits / decoder states come back with B * G rows."""
        G = check_targets_per_input(targets_per_input, input_ids, decoder_input_ids=decoder_input_ids,
                                    decoder_attention_mask=decoder_attention_mask, labels=labels)
        with torch.cuda.device(self.device):
            b, keep, (B, S, T, ntot) = self._batch(input_ids, image_features if encoder_states is None else [],
                                                   attention_mask, decoder_input_ids, decoder_attention_mask, labels)
            Bd = B * G   # decoder rows
            if G > 1:
                self._ensure_ws(self.lib.kmb_workspace_bytes_grouped(self.h, B, S, T, ntot, G))
            else:
                self._ensure_ws(self.lib.kmb_workspace_bytes(self.h, B, S, T, ntot))
            self._poison()
            D = int(self.config.d_model)
            logits = None
            if want_logits:
                logits = torch.empty((Bd * T, self.logits_ld), dtype=torch.float32, device=self.device)
            enc = None
            if want_encoder:
                enc = torch.empty((B, S, D), dtype=self.act_dtype, device=self.device)
            loss = torch.empty(1, dtype=torch.float32, device=self.device) if labels is not None else None
            opts = KmbForwardOpts()
            dec = None
            if encoder_states is not None:
                if tuple(encoder_states.shape) != (B, S, D):
                    raise ValueError("encoder_outputs[0] must be [batch, src_len, d_model] = %s, got %s"
                                     % ((B, S, D), tuple(encoder_states.shape)))
                encoder_states = encoder_states.to(device=self.device, dtype=self.act_dtype).contiguous()
                opts.encoder_states = ptr(encoder_states)
                keep.append(encoder_states)
            if want_decoder_states:
                dec = torch.empty((Bd, T, D), dtype=self.act_dtype, device=self.device)
                opts.decoder_states_out = ptr(dec)
            opts.skip_head = 1 if skip_head else 0
            self._loss_opts(opts, keep, loss_weights, loss_reduction, labels, Bd, T)
            if G > 1:
                opts.targets_per_input = G
            self.fwd_serial += 1
            check(self.lib.kmb_forward_ex(self.h, C.byref(b), C.byref(opts), 1 if train else 0, 1 if need_grad else 0,
                                          ptr(loss), ptr(logits), ptr(enc), _stream()))
            self._keep = keep
            if logits is not None:
                logits = logits.view(Bd, T, self.logits_ld)[:, :, : int(self.config.vocab_size)]
            self._last_bt = (B, T)
            self._last_bd = Bd
            self._last_S = S
            return (loss, logits, enc, dec) if want_decoder_states else (loss, logits, enc)

    def score(self, input_ids, image_features, attention_mask=None, decoder_input_ids=None, decoder_attention_mask=None,
              labels=None):
        """log p(label | image, event, earlier labels) of a GIVEN target sequence (kmb_score; reference
        scripts/filter_reason.py:24-52 without the [B, T, V] logits).  Returns device tensors (token_logprobs fp32 [B, T], nll fp32 [B]
        -- a sum --, count int32 [B]); no host synchronisation.  `last_score_path` is 1 when the store-free head ran, 0 for the
        fallback (KMB_SCORE_FALLBACK=1 forces it)."""
        if labels is None:
            raise ValueError("score() needs labels: the sequence to score")
        with torch.cuda.device(self.device):
            b, keep, (B, S, T, ntot) = self._batch(input_ids, image_features, attention_mask, decoder_input_ids,
                                                   decoder_attention_mask, labels)
            self._ensure_ws(self.lib.kmb_workspace_bytes(self.h, B, S, T, ntot))
            self._poison()
            logp = torch.empty((B, T), dtype=torch.float32, device=self.device)
            nll = torch.empty(B, dtype=torch.float32, device=self.device)
            count = torch.empty(B, dtype=torch.int32, device=self.device)
            path = C.c_int32(-1)
            self.fwd_serial += 1
            check(self.lib.kmb_score(self.h, C.byref(b), ptr(logp), ptr(nll), ptr(count), C.byref(path), _stream()))
            self._keep = keep
            self._last_bt = (B, T)
            self._last_bd = B
            self._last_S = S
            self.last_score_path = int(path.value)
            return logp, nll, count

    def hidden_states(self, which):
        """`output_hidden_states` of the forward still in the workspace: tuple of [B, T, d] activations of the encoder
        (which = 0: embedding output + every layer's output) or decoder (which = 1) stack."""
        B, T = self._last_bt
        if which == 1:
            B = getattr(self, "_last_bd", B)   # decoder rows: B * targets_per_input
        rows_T = T if which == 1 else self._last_S
        n = int(self.config.encoder_layers if which == 0 else self.config.decoder_layers) + 1
        out = []
        with torch.cuda.device(self.device):
            for i in range(n):
                t = torch.empty((B, rows_T, int(self.config.d_model)), dtype=torch.bfloat16, device=self.device)
                check(self.lib.kmb_hidden_state(self.h, which, i, ptr(t), _stream()))
                out.append(t)
        return tuple(out)

    def encoder_last_state(self):
        """[B, S, d] bf16: the encoder output of the forward still in the workspace (what want_encoder=True copies eagerly)."""
        B, _ = self._last_bt
        t = torch.empty((B, self._last_S, int(self.config.d_model)), dtype=torch.bfloat16, device=self.device)
        with torch.cuda.device(self.device):
            check(self.lib.kmb_hidden_state(self.h, 0, int(self.config.encoder_layers), ptr(t), _stream()))
        return t

    def encoder_states_grad(self):
        """dL / d(encoder output) of the backward that just ran, bf16 [B, S, d]: what autograd hands to a tensor passed as
        `encoder_outputs` (src/model/model.py:76-83)."""
        B, _ = self._last_bt
        t = torch.empty((B, self._last_S, int(self.config.d_model)), dtype=torch.bfloat16, device=self.device)
        with torch.cuda.device(self.device):
            check(self.lib.kmb_encoder_states_grad(self.h, ptr(t), _stream()))
        return t

    def attention_probs(self, which):
        """`output_attentions`: tuple over layers of fp32 [B, H, T, T] self-attention probabilities."""
        B, T = self._last_bt
        Tq = T if which == 1 else self._last_S
        H = int(self.config.encoder_attention_heads if which == 0 else self.config.decoder_attention_heads)
        n = int(self.config.encoder_layers if which == 0 else self.config.decoder_layers)
        out = []
        with torch.cuda.device(self.device):
            for l in range(n):
                t = torch.empty((B, H, Tq, Tq), dtype=torch.float32, device=self.device)
                check(self.lib.kmb_attention_probs(self.h, which, l, ptr(t), _stream()))
                out.append(t)
        return tuple(out)

    def last_logits(self):
        """fp32 logits [B,T,V] of the decoder states the last forward left in the workspace (one head GEMM)."""
        B, T = self._last_bt
        B = getattr(self, "_last_bd", B)   # decoder rows: B * targets_per_input
        with torch.cuda.device(self.device):
            logits = torch.empty((B * T, self.logits_ld), dtype=torch.float32, device=self.device)
            check(self.lib.kmb_last_logits(self.h, ptr(logits), _stream()))
        return logits.view(B, T, self.logits_ld)[:, :, : int(self.config.vocab_size)]

    def forward_pretrain(self, input_ids, image_features, attention_mask, decoder_input_ids, decoder_attention_mask,
                         labels, mrm=None, attr=None, rel=None, factors=(1.0, 1.0, 1.0, 1.0), train=False,
                         need_grad=False, want_logits=False, encoder_states=None, want_encoder=False,
                         loss_weights=None, loss_reduction="mean"):
        """mrm = (rows int32 [n], soft targets fp32 [n, C]); attr = (rows, labels int64); rel = (obj rows, subj rows,
        labels).  Returns (losses fp32 [5] = total, lm, mrm, attribute, relation; logits or None) -- plus the encoder states
        with want_encoder.  `encoder_states` [B,S,D] skips the encoder (reference src/model/model.py:225-242 passes
        `encoder_outputs` through to self.model).  `loss_weights` / `loss_reduction` as in `forward`: the LM term only."""
        refuse_ignored_head_labels("attribute", None if attr is None else attr[1])
        refuse_ignored_head_labels("relation", None if rel is None else rel[2])
        with torch.cuda.device(self.device):
            b, keep, (B, S, T, ntot) = self._batch(input_ids, image_features if encoder_states is None else [], attention_mask,
                                                   decoder_input_ids, decoder_attention_mask, labels)
            dev = self.device

            def i32(t):
                return t.to(device=dev, dtype=torch.int32).contiguous()

            ex = KmbPretrain(lm_factor=factors[0], mrm_factor=factors[1], attr_factor=factors[2], rel_factor=factors[3])
            nmax = 0
            if mrm is not None and mrm[0].numel() > 0:
                rows, tgt = i32(mrm[0]), mrm[1].to(device=dev, dtype=torch.float32).contiguous()
                ex.n_mrm, ex.mrm_rows, ex.mrm_targets = rows.numel(), ptr(rows), ptr(tgt)
                keep += [rows, tgt]
                nmax = max(nmax, rows.numel())
            if attr is not None and attr[0].numel() > 0:
                rows, lab = i32(attr[0]), attr[1].to(device=dev, dtype=torch.int64).contiguous()
                ex.n_attr, ex.attr_rows, ex.attr_labels = rows.numel(), ptr(rows), ptr(lab)
                keep += [rows, lab]
                nmax = max(nmax, rows.numel())
            if rel is not None and rel[0].numel() > 0:
                ro, rs, lab = i32(rel[0]), i32(rel[1]), rel[2].to(device=dev, dtype=torch.int64).contiguous()
                ex.n_rel, ex.rel_obj_rows, ex.rel_subj_rows, ex.rel_labels = ro.numel(), ptr(ro), ptr(rs), ptr(lab)
                keep += [ro, rs, lab]
                nmax = max(nmax, ro.numel())
            check(self.lib.kmb_reserve_head_rows(self.h, max(nmax, 8)))
            self._ensure_ws(self.lib.kmb_workspace_bytes(self.h, B, S, T, ntot))
            self._poison()
            losses = torch.zeros(5, dtype=torch.float32, device=dev)
            ex.losses_out = ptr(losses)
            logits = torch.empty((B * T, self.logits_ld), dtype=torch.float32, device=dev) if want_logits else None
            self.fwd_serial += 1
            self._last_bt = (B, T)
            self._last_bd = B
            self._last_S = S
            D = int(self.config.d_model)
            opts = KmbForwardOpts()
            if encoder_states is not None:
                if tuple(encoder_states.shape) != (B, S, D):
                    raise ValueError("encoder_outputs[0] must be [batch, src_len, d_model] = %s, got %s"
                                     % ((B, S, D), tuple(encoder_states.shape)))
                encoder_states = encoder_states.to(device=dev, dtype=self.act_dtype).contiguous()
                opts.encoder_states = ptr(encoder_states)
                keep.append(encoder_states)
            enc = torch.empty((B, S, D), dtype=self.act_dtype, device=dev) if want_encoder else None
            self._loss_opts(opts, keep, loss_weights, loss_reduction, labels, B, T)
            check(self.lib.kmb_forward_pretrain_ex(self.h, C.byref(b), C.byref(ex), C.byref(opts), 1 if train else 0,
                                                   1 if need_grad else 0, ptr(logits), ptr(enc), _stream()))
            self._keep = keep
            if logits is not None:
                logits = logits.view(B, T, self.logits_ld)[:, :, : int(self.config.vocab_size)]
            return (losses, logits, enc) if want_encoder else (losses, logits)

    def check_inputs(self):
        """Raises if the device-side validation of the last forward flagged the batch (syncs)."""
        st = C.c_int32(0)
        with torch.cuda.device(self.device):
            check(self.lib.kmb_read_status(self.h, C.byref(st), _stream()))
        self._raise_on_status(st.value)

    @staticmethod
    def _raise_on_status(st):
        if st & 1:
            raise RuntimeError("number of <img_feat>/<cls> ids differs from the number of region features "
                               "(reference src/model/modules.py:98-100 would raise a shape mismatch)")
        if st & 2:
            raise RuntimeError("a label is neither -100 nor inside [0, number of classes) "
                               "(the reference's CrossEntropyLoss raises on such a target, src/model/model.py:400-402)")

    def read_status(self):
        """The device status word of the last forward / generation (syncs); bits: _raise_on_status."""
        st = C.c_int32(0)
        with torch.cuda.device(self.device):
            check(self.lib.kmb_read_status(self.h, C.byref(st), _stream()))
        return int(st.value)

    def check_inputs_begin(self):
        """check_inputs without the wait: the status word is copied to page-locked memory in stream order; the caller
        calls check_inputs_end() after its next synchronisation of the stream."""
        st = self.pinned((1,), torch.int32)
        with torch.cuda.device(self.device):
            check(self.lib.kmb_read_status_async(self.h, ptr(st), _stream()))
            ev = torch.cuda.Event()
            ev.record()
        self._status_pending = (st, ev)

    def check_inputs_end(self):
        pend = self.__dict__.pop("_status_pending", None)
        if pend is None:
            return
        st, ev = pend
        ev.synchronize()
        self._raise_on_status(int(st[0]))

    def backward(self, loss_scale=1.0):
        """loss_scale: a Python float, or a 1-element fp32 device tensor (autograd's upstream gradient: no host sync)."""
        with torch.cuda.device(self.device):
            if torch.is_tensor(loss_scale):
                sc = loss_scale.detach().to(device=self.device, dtype=torch.float32).reshape(1).contiguous()
                check(self.lib.kmb_backward_dev(self.h, ptr(sc), _stream()))
                self._keep_scale = sc
            else:
                check(self.lib.kmb_backward(self.h, C.c_float(loss_scale), _stream()))

    # ---- gradient accumulation over micro-batches (kmb_set_grad_accumulation, include/kmbart.h) ---------------------------
    def grad_accumulation(self, on=True):
        """on: a backward leaves its micro-batch's gradient in the stage (a second arena, allocated here on first use: 4 B per
        parameter) and folds it into `grads` bucket by bucket, overwriting on the first backward after zero_grad() and adding
        afterwards; `grads` -- what the optimizer, the norm, the data-parallel exchange and `p.grad` read -- holds the running
        total.  off: every backward overwrites `grads` directly (the default).  Not between a need_grad forward and its backward."""
        with torch.cuda.device(self.device):
            if on and getattr(self, "_grad_stage", None) is None:
                self._grad_stage = torch.zeros(self.n, dtype=torch.float32, device=self.device)
                check(self.lib.kmb_bind_grad_stage(self.h, ptr(self._grad_stage), self._grad_stage.numel()))
            check(self.lib.kmb_set_grad_accumulation(self.h, 1 if on else 0))
        self.accumulating = bool(on)

    accumulating = False

    def zero_grad(self):
        """The next backward starts a new sum (a host flag: nothing is launched, `grads` keeps its values until then).  No
        effect while accumulation is off."""
        check(self.lib.kmb_zero_grad(self.h))

    @property
    def grad_stage(self):
        """The stage as a tensor (the LAST backward's own gradient while accumulation is on), None before grad_accumulation(True)."""
        return getattr(self, "_grad_stage", None)

    def adamw_step(self, lr, betas=(0.9, 0.999), eps=1e-6, weight_decay=0.0, correct_bias=True, grad_scale=1.0,
                   offset=0, count=None, bump=True):
        if bump:
            self.step_count += 1
        self.fwd_serial += 1   # the weights move: logits of an earlier forward can no longer be reproduced
        hp = KmbAdamW(lr=lr, beta1=betas[0], beta2=betas[1], eps=eps, weight_decay=weight_decay,
                      step=self.step_count, correct_bias=1 if correct_bias else 0, grad_scale=grad_scale)
        with torch.cuda.device(self.device):
            check(self.lib.kmb_adamw_step(self.h, C.byref(hp), offset, self.n - offset if count is None else count,
                                          _stream()))

    def adamw_step_overlapped(self, lr, betas=(0.9, 0.999), eps=1e-6, weight_decay=0.0, correct_bias=True, grad_scale=1.0,
                              offset=0, count=None):
        """The same update issued per gradient bucket on a second stream, each launch behind that bucket's completion
        event of the backward pass that is still executing on the GPU (the host enqueues a step in ~2 ms, the GPU needs
        ~20 ms for backward): the HBM-bound update of the decoder and encoder layers runs beside the compute-bound rest of
        backward; only the tied matrix (last bucket) is left for after it.  Parameters of a bucket are not read again by
        the backward pass once its event is recorded.  Returns False (nothing issued) when a piece is not 8-aligned or a
        data-parallel reducer owns the gradients (they are final only after its all-reduce)."""
        if not getattr(self, "adamw_overlap_ok", True):
            return False
        count = self.n - offset if count is None else count
        if getattr(self, "_bucket_list", None) is None:
            self._bucket_list = self.buckets()
            self._opt_stream = torch.cuda.Stream(device=self.device)
        end = offset + count
        pieces = []
        for i, (boff, bcnt) in enumerate(self._bucket_list):
            lo, hi = max(offset, boff), min(end, boff + bcnt)
            if lo < hi:
                if lo & 7:
                    return False
                pieces.append((i, lo, hi - lo))
        if sum(c for _, _, c in pieces) != count:
            return False
        hp = KmbAdamW(lr=lr, beta1=betas[0], beta2=betas[1], eps=eps, weight_decay=weight_decay,
                      step=self.step_count, correct_bias=1 if correct_bias else 0, grad_scale=grad_scale)
        self.fwd_serial += 1
        with torch.cuda.device(self.device):
            main, side = torch.cuda.current_stream(), self._opt_stream
            for i, lo, cnt in pieces:
                self.stream_wait_bucket(i, side)
                check(self.lib.kmb_adamw_step(self.h, C.byref(hp), lo, cnt, C.c_void_p(side.cuda_stream)))
            main.wait_stream(side)
        return True

    # ---- clipped / guarded optimizer step (kmbart.optim.AdamW(max_grad_norm=..., skip_nonfinite=...)) ------------------
    def bind_step_state(self):
        """The step's device record (KmbStepState) and the partial sums of the gradient norm: a buffer of its own, NOT part of
        the workspace (KMB_POISON rewrites that before every forward; the bias-correction step count lives here).  Bound once;
        the device step count starts at the host's."""
        if getattr(self, "_step_buf", None) is None:
            with torch.cuda.device(self.device):
                buf = torch.zeros(int(self.lib.kmb_step_state_bytes(self.h)), dtype=torch.uint8, device=self.device)
                torch.cuda.synchronize(self.device)
                check(self.lib.kmb_bind_step_state(self.h, ptr(buf), buf.numel()))
                check(self.lib.kmb_step_state_set_steps(self.h, int(self.step_count), _stream()))
            self._step_buf = buf
            self._steps_written = True   # on the caller's stream: see guarded_step
            self._step_host = torch.zeros(C.sizeof(_lib.KmbStepState), dtype=torch.uint8).pin_memory()
        return self._step_buf

    def step_pieces(self, ranges):
        """[(bucket, offset, count, slot0)] in ascending offset order: the (offset, count) ranges cut at the gradient buckets'
        boundaries, each with its own block of partial slots -- the same pieces, hence the same bits, whichever stream
        sums them.  The second value is the number of slots in use."""
        if getattr(self, "_bucket_list", None) is None:
            self._bucket_list = self.buckets()
            self._opt_stream = torch.cuda.Stream(device=self.device)
        pieces = []
        for off, cnt in ranges:
            for i, (boff, bcnt) in enumerate(self._bucket_list):
                lo, hi = max(off, boff), min(off + cnt, boff + bcnt)
                if lo < hi:
                    pieces.append((i, lo, hi - lo))
        if sum(c for _, _, c in pieces) != sum(c for _, c in ranges):
            raise _lib.KmbError("the optimizer's parameter ranges are not covered by the engine's gradient buckets")
        pieces.sort(key=lambda x: x[1])
        out, slot = [], 0
        for i, lo, cnt in pieces:
            out.append((i, lo, cnt, slot))
            slot += int(self.lib.kmb_op_grad_sumsq_slots(cnt))
        return out, slot

    def guarded_step(self, groups, max_norm, skip_nonfinite, grad_scale=1.0, overlap=False):
        """Sum of squares of every piece -> ONE finish launch (norm, clip coefficient, finite?, step size: the KmbStepState
        record) -> the device-state AdamW of every piece.  groups: [(hyperparameter dict, [(offset, count)])].  overlap: each
        piece's sum goes on the optimizer's side stream behind its bucket's completion event of the backward pass still
        running on the GPU; the finish launch and the updates follow on that stream (the norm needs every gradient, so they
        cannot start earlier) and the caller's stream waits for it.  Nothing here synchronises the host."""
        self.bind_step_state()
        # the pieces, their slots and each piece's parameter group are constant for a given set of ranges: built once
        key = tuple((off, cnt, gi) for gi, (_, ranges) in enumerate(groups) for off, cnt in ranges)
        plan = getattr(self, "_step_plan", None)
        if plan is None or plan[0] != key:
            pieces, nslots = self.step_pieces([(off, cnt) for off, cnt, _ in key])
            owner = [next(gi for off, cnt, gi in key if off <= lo < off + cnt) for _, lo, _, _ in pieces]
            plan = self._step_plan = (key, pieces, nslots, owner, sorted(pieces, key=lambda x: x[0]))
        _, pieces, nslots, owner, by_bucket = plan
        if overlap and not getattr(self, "adamw_overlap_ok", True):
            overlap = False
        hps = [KmbAdamW(lr=g["lr"], beta1=g["betas"][0], beta2=g["betas"][1], eps=g["eps"], weight_decay=g["weight_decay"],
                        step=0, correct_bias=1 if g["correct_bias"] else 0, grad_scale=grad_scale) for g, _ in groups]
        self.fwd_serial += 1   # the weights move
        with torch.cuda.device(self.device):
            main = torch.cuda.current_stream()
            side = self._opt_stream if overlap else main
            s = C.c_void_p(side.cuda_stream)
            if overlap and self._steps_written:
                # the record's step count was written on the caller's stream (first bind, set_device_steps), possibly behind the
                # backward pass whose bucket events are all the side stream waits for: order the finish launch behind that write
                side.wait_stream(main)
            self._steps_written = False
            # launch order = bucket completion order (what backward finishes first is summed first); the slots do not depend on it
            for i, lo, cnt, slot0 in by_bucket:
                if overlap:
                    self.stream_wait_bucket(i, side)
                check(self.lib.kmb_grad_sumsq(self.h, lo, cnt, C.c_float(grad_scale), slot0, s))
            check(self.lib.kmb_clip_finish(self.h, C.byref(hps[0]), C.c_float(max_norm if max_norm is not None else 0.0),
                                           1 if skip_nonfinite else 0, nslots, s))
            for (i, lo, cnt, _), gi in zip(pieces, owner):
                check(self.lib.kmb_adamw_step_dev(self.h, C.byref(hps[gi]), lo, cnt, s))
            if overlap:
                main.wait_stream(side)

    @property
    def grad_norm(self):
        """0-d fp32 device view of the record's `norm` (the last guarded step's pre-clip global gradient norm): no sync."""
        return self.bind_step_state()[:4].view(torch.float32).view(())

    def step_state(self):
        """The record on the host (synchronises)."""
        self.bind_step_state()
        with torch.cuda.device(self.device):
            check(self.lib.kmb_step_state_read(self.h, C.c_void_p(self._step_host.data_ptr()), _stream()))
            torch.cuda.current_stream().synchronize()
        return StepRecord.decode(self._step_host)

    def step_record(self):
        """A device copy of the record in stream order (no synchronisation); StepRecord.read() brings it to the host later."""
        return StepRecord(self.bind_step_state()[:C.sizeof(_lib.KmbStepState)].clone())

    def set_device_steps(self, steps):
        self.bind_step_state()
        with torch.cuda.device(self.device):
            check(self.lib.kmb_step_state_set_steps(self.h, int(steps), _stream()))
        self._steps_written = True

    # ---- data-parallel buckets --------------------------------------------------------------
    def buckets(self):
        out = []
        off, cnt = C.c_int64(), C.c_int64()
        for i in range(self.lib.kmb_bucket_count(self.h)):
            check(self.lib.kmb_bucket_range(self.h, i, C.byref(off), C.byref(cnt)))
            out.append((off.value, cnt.value))
        return out

    def stream_wait_bucket(self, i, stream):
        check(self.lib.kmb_stream_wait_bucket(self.h, i, C.c_void_p(stream.cuda_stream)))

    # ---- native RCCL gradient exchange (kmb_comm_*, include/kmbart.h) ------------------------
    def comm_init(self, process_group=None):
        """Creates the library's own RCCL communicator over the ranks of `process_group` (torch.distributed is only the
        bootstrap channel for the 128-byte id, as torchrun's rendezvous is for init_process_group in the reference,
        src/utils.py:9-17).  Returns (rank, world)."""
        import torch.distributed as dist
        rank, world = dist.get_rank(process_group), dist.get_world_size(process_group)
        box = [None]
        if rank == 0:
            buf = C.create_string_buffer(128)
            check(self.lib.kmb_comm_unique_id(buf))
            box[0] = bytes(buf.raw)
        src = dist.get_global_rank(process_group, 0) if process_group is not None else 0
        dist.broadcast_object_list(box, src=src, group=process_group)
        with torch.cuda.device(self.device):
            check(self.lib.kmb_comm_init(self.h, rank, world, C.c_char_p(box[0])))
        self.comm_world = world
        return rank, world

    def comm_destroy(self):
        """Drops the library's communicator (the data-parallel wrapper's fallback to torch.distributed when the native
        bootstrap failed on another rank).  If a reduce-scatter exchange left exp_avg / exp_avg_sq sharded, they are gathered first
        (a COLLECTIVE: teardown runs on every rank; after a failed bootstrap nothing is sharded) -- kmb_comm_destroy clears the flag."""
        with torch.cuda.device(self.device):
            if self.moments_sharded:
                check(self.lib.kmb_comm_gather_moments(self.h, _stream()))
                torch.cuda.synchronize(self.device)
            check(self.lib.kmb_comm_destroy(self.h))
        self.comm_world = 0

    def comm_broadcast_params(self, root=0):
        with torch.cuda.device(self.device):
            check(self.lib.kmb_comm_broadcast_params(self.h, int(root), _stream()))

    def allreduce_grads(self, algo=0, adamw=None, max_piece_elems=0, after_compute=False):
        """One call = the whole gradient exchange of a step on the library's communication stream (mean over ranks per
        bucket behind its completion event, optionally each piece's fused AdamW behind it).  adamw: KmbAdamW or None."""
        from ._lib import KmbAllreduceOpts
        o = KmbAllreduceOpts(algo=int(algo), after_compute=1 if after_compute else 0, max_piece_elems=int(max_piece_elems),
                             adamw=C.pointer(adamw) if adamw is not None else None)
        with torch.cuda.device(self.device):
            check(self.lib.kmb_allreduce_grads(self.h, C.byref(o), _stream()))
        if adamw is not None:
            self.fwd_serial += 1   # the weights move

    def comm_wait(self):
        with torch.cuda.device(self.device):
            check(self.lib.kmb_comm_wait(self.h, _stream()))

    def comm_gather_moments(self):
        """COLLECTIVE (every rank must call it): all-gathers the shards of exp_avg / exp_avg_sq that an algo-1 exchange with a
        fused optimizer leaves current on their owning rank only."""
        with torch.cuda.device(self.device):
            check(self.lib.kmb_comm_gather_moments(self.h, _stream()))

    @property
    def moments_sharded(self):
        """True after a reduce-scatter exchange with a fused optimizer on more than one rank, until comm_gather_moments()."""
        return bool(self.lib.kmb_comm_moments_sharded(self.h))

    def comm_plan(self, world, rank, max_piece_elems=0):
        """The exchange's partition as rank `rank` of `world` sees it (kmb_comm_plan: a pure host function, no communicator
        needed): list of dicts bucket / offset / count / shard / mine / repad_piece / repad_shard."""
        from ._lib import KmbCommPiece
        out = []
        for i in range(int(self.lib.kmb_comm_pieces(self.h, int(max_piece_elems)))):
            pc = KmbCommPiece()
            check(self.lib.kmb_comm_plan(self.h, int(world), int(rank), int(max_piece_elems), i, C.byref(pc)))
            out.append({k: int(getattr(pc, k)) for k in ("bucket", "offset", "count", "shard", "mine", "repad_piece", "repad_shard")})
        return out

    # ---- generation -------------------------------------------------------------------------
    def set_gen_weight_format(self, name):
        """The format of the six per-layer decoder matrices the fused decode blocks read: "bf16" (default) or "fp8_e4m3" (OCP e4m3
        codes with a power-of-two scale per weight row: half the weight bytes of a decode step).  Read by gen_begin and the decode
        steps only.  FP8 exists only where the fused blocks run; anything else raises, here or in gen_begin (kmb_gen_set_weight_format)."""
        if name not in _lib.WEIGHT_FORMATS:
            raise ValueError("decoder weight format must be one of %s, got %r" % (sorted(_lib.WEIGHT_FORMATS), name))
        if name == self.gen_weight_format:
            return
        torch.cuda.synchronize(self.device)   # the packed copies of a generation still in flight are about to be resized
        check(self.lib.kmb_gen_set_weight_format(self.h, _lib.WEIGHT_FORMATS[name]))
        self.gen_weight_format = name

    def gen_begin(self, input_ids, image_features, attention_mask, num_beams, max_length):
        with torch.cuda.device(self.device):
            b, keep, (B, S, _, ntot) = self._batch(input_ids, image_features, attention_mask, None, None, None)
            self._ensure_ws(self.lib.kmb_gen_workspace_bytes(self.h, B, S, num_beams, max_length, ntot))
            self._poison()
            self.fwd_serial += 1
            check(self.lib.kmb_gen_begin(self.h, C.byref(b), num_beams, max_length, _stream()))
            self._keep = keep
            self._gen_rows = B * num_beams
            self._gen_enc_shape = (B, S)
            self._gen_max_length = int(max_length)
            self._gen_logits = torch.empty((self._gen_rows, self.logits_ld), dtype=torch.float32, device=self.device)
            self._gen_logits_version = None   # _gen_logits._version right after the last gen_step that wrote them
            self._folded = None               # (ntok, its _version, step): the tokens the last beam_step embedded for that step

    def gen_encoder_states(self):
        """[B, S, d] bf16: the encoder output of the active gen_begin (a copy)."""
        B, S = self._gen_enc_shape
        out = torch.empty((B, S, int(self.config.d_model)), dtype=torch.bfloat16, device=self.device)
        with torch.cuda.device(self.device):
            check(self.lib.kmb_gen_encoder_states(self.h, ptr(out), _stream()))
        return out

    def gen_step(self, tokens, step, want_logits=True):
        """tokens int64 [B*num_beams] (device) at 0-based position `step` -> fp32 logits [R, V] (padded view).
        want_logits=False: the decoder layers run (the KV cache gets position `step`) but the vocabulary projection is
        skipped; the returned buffer then holds stale values (for steps whose token is forced).
        When `tokens` is the very next_tokens tensor the last beam_step(reorder_step = step - 1) returned, unchanged since (same
        _version), and that beam step embedded them, the step runs on that embedding (kmb_gen_step with tokens = NULL, no
        embedding launch); any other tokens are embedded.  (Writes to that tensor that torch does not see -- a raw pointer
        handed to other native code -- are the caller's to avoid.)"""
        folded, self._folded = self.__dict__.get("_folded"), None
        with torch.cuda.device(self.device):
            if folded is not None and tokens is folded[0] and tokens._version == folded[1] and int(step) == folded[2]:
                tok_ptr = None
            else:
                tokens = tokens.to(device=self.device, dtype=torch.int64).contiguous()
                tok_ptr = ptr(tokens)
            check(self.lib.kmb_gen_step(self.h, tok_ptr, int(step), ptr(self._gen_logits) if want_logits else None, _stream()))
            self._keep_tok = tokens
        self._gen_logits_version = self._gen_logits._version if want_logits else None
        return self._gen_logits

    def gen_last_hidden(self):
        """[rows, d] bf16: the final decoder states of the last gen_step (kmb_gen_last_hidden)."""
        out = torch.empty((self._gen_rows, int(self.config.d_model)), dtype=torch.bfloat16, device=self.device)
        with torch.cuda.device(self.device):
            check(self.lib.kmb_gen_last_hidden(self.h, ptr(out), _stream()))
        return out

    def gen_reorder(self, beam_idx, step):
        with torch.cuda.device(self.device):
            beam_idx = beam_idx.to(device=self.device, dtype=torch.int32).contiguous()
            check(self.lib.kmb_gen_reorder(self.h, ptr(beam_idx), int(step), _stream()))
            self._keep_idx = beam_idx

    def beam_candidates(self, logits, num_beams, k, add=None, force_token=-1, ban_token=-1):
        """log_softmax(+beam score) top-k per beam row, merged per batch item: int32 [B, k, 2] on the device,
        [..., 0] = fp32 score bits, [..., 1] = beam * V + token (one small D2H copy per decode step)."""
        R = logits.shape[0]
        val, idx = self.logsoftmax_topk(logits, k, add=add, force_token=force_token, ban_token=ban_token)
        out = torch.empty((R // num_beams, k, 2), dtype=torch.int32, device=self.device)
        with torch.cuda.device(self.device):
            check(self.lib.kmb_beam_merge(ptr(val), ptr(idx), R // num_beams, int(num_beams), int(k),
                                          int(self.config.vocab_size), ptr(out), _stream()))
        return out

    def pinned(self, shape, dtype):
        """A cached page-locked host tensor (asynchronous device-to-host staging)."""
        key = (tuple(shape), dtype)
        cache = self.__dict__.setdefault("_pinned", {})
        if key not in cache:
            cache[key] = torch.empty(shape, dtype=dtype, pin_memory=True)
        return cache[key]

    def _beam_outputs(self, cand_out, B, k, R):
        """The outputs of a beam step: (cand int32 [B, k, 2], next_scores fp32 [R], next_tokens int64 [R], next_beam_idx int32 [R]).
        cand_out: a page-locked host tensor [B, k, 2] int32 the kernel writes directly (device-visible host memory: no copy launch
        between two decode steps); the caller reads it after an event recorded behind the call."""
        self._folded = None
        cand = cand_out if cand_out is not None else torch.empty((B, k, 2), dtype=torch.int32, device=self.device)
        nscore = torch.empty((R,), dtype=torch.float32, device=self.device)
        ntok = torch.empty((R,), dtype=torch.int64, device=self.device)
        nidx = torch.empty((R,), dtype=torch.int32, device=self.device)
        return cand, nscore, ntok, nidx

    def _beam_call(self, logits, outs, reorder_step, gen_call, call, forced=False):
        """Runs a beam step: gen_call (its kmb_gen_* form: the decode loop's, which may select from the statistics the step's
        vocabulary projection left and folds the reorder and the next step's embedding into its launch) when `logits` are
        gen_step's, unedited since (their _version unchanged; a forced step reads none), else `call` (the stateless form)
        and then gen_reorder.  gen_call None: the stateless form only."""
        nidx, ntok = outs[3], outs[2]
        with torch.cuda.device(self.device):
            if (gen_call is not None and logits is self.__dict__.get("_gen_logits")
                    and (forced or logits._version == self._gen_logits_version)):
                check(gen_call())
                self._keep_idx = nidx
                if reorder_step >= 0 and self.lib.kmb_gen_embedded_step(self.h) == reorder_step + 1:
                    self._folded = (ntok, ntok._version, reorder_step + 1)
                return outs
            check(call())
        if reorder_step >= 0:
            self.gen_reorder(nidx, reorder_step)
        return outs

    def beam_step(self, logits, num_beams, k, add, force_token=-1, ban_token=-1, eos_token=-1, cand_out=None, reorder_step=-1):
        """beam_candidates plus the next step's beams chosen on the device (kmb_beam_merge_select): returns
        (cand int32 [B, k, 2], next_scores fp32 [R], next_tokens int64 [R], next_beam_idx int32 [R]); nothing is
        copied to the host.  `add` may be one of the returned next_scores (stream order makes that safe).
        reorder_step >= 0: the call also reorders the generation caches by next_beam_idx (gen_reorder(next_beam_idx,
        reorder_step), folded into the beam step's launch when `logits` are gen_step's)."""
        R = logits.shape[0]
        B = R // num_beams
        outs = cand, nscore, ntok, nidx = self._beam_outputs(cand_out, B, k, R)
        if k <= 16 and num_beams <= 16 and num_beams * k <= 256 and logits.stride(0) % 4 == 0:
            # kmb_beam_step: the rows' top-k lists never leave the workgroup that merges them (one launch less per decode step)
            scr = self._topk_scratch_for(R)
            return self._beam_call(
                logits, outs, reorder_step,
                lambda: self.lib.kmb_gen_beam_step(self.h, ptr(logits), logits.stride(0), int(num_beams), ptr(add), int(force_token),
                                                   int(ban_token), int(k), ptr(cand), int(eos_token), ptr(nscore), ptr(ntok),
                                                   ptr(nidx), ptr(scr), scr.numel(), int(reorder_step), _stream()),
                lambda: self.lib.kmb_beam_step(ptr(logits), logits.stride(0), int(self.config.vocab_size), B, int(num_beams), ptr(add),
                                               int(force_token), int(ban_token), int(k), ptr(cand), int(eos_token), ptr(nscore),
                                               ptr(ntok), ptr(nidx), ptr(scr), scr.numel(), _stream()),
                forced=force_token >= 0)
        val, idx = self.logsoftmax_topk(logits, k, add=add, force_token=force_token, ban_token=ban_token)
        return self._beam_call(
            logits, outs, reorder_step, None,
            lambda: self.lib.kmb_beam_merge_select(ptr(val), ptr(idx), B, int(num_beams), int(k), int(self.config.vocab_size),
                                                   ptr(cand), int(eos_token), ptr(nscore), ptr(ntok), ptr(nidx), _stream()))

    def beam_step_processed(self, logits, num_beams, k, add, ids_in, ids_out, t, repetition_penalty=1.0, no_repeat_ngram_size=0,
                            bad_words=None, force_token=-1, ban_token=-1, eos_token=-1, cand_out=None, reorder_step=-1):
        """beam_step with generate()'s score processors applied to the rows' log-probabilities on the device
        (kmb_beam_step_processed; its decode-loop form when `logits` are gen_step's): repetition penalty, no-repeat n-grams and
        bad words from the beams' tokens ids_in[:, :t] (int64 [R, ld]); bad_words: (tokens int32, offsets int32 [n_bad + 1])
        device tensors, the packed table, or None.  ids_out (int64 [R, ld], another buffer) receives the next beams' histories,
        columns [0, t].  Returns beam_step's tuple; reorder_step as there.  Shapes outside the fused beam step's limits raise."""
        R, V = logits.shape[0], int(self.config.vocab_size)
        B = R // num_beams
        assert logits.device == self.device and logits.dtype == torch.float32 and logits.dim() == 2 and logits.stride(1) == 1, \
            "beam_step_processed: bad logits"
        for x in (ids_in, ids_out):
            assert x.device == self.device and x.dtype == torch.int64 and x.dim() == 2 and x.stride(1) == 1 and x.shape[0] == R, \
                "beam_step_processed: bad ids"
        assert ids_in.stride(0) == ids_out.stride(0) and ids_in.data_ptr() != ids_out.data_ptr(), "beam_step_processed: bad ids"
        btok = boff = None
        n_bad = 0
        if bad_words is not None:
            btok, boff = bad_words
            for x in (btok, boff):
                assert x.device == self.device and x.dtype == torch.int32 and x.is_contiguous(), "beam_step_processed: bad table"
            n_bad = boff.numel() - 1
            assert n_bad >= 0 and (n_bad == 0 or btok.numel() > 0)
        outs = cand, nscore, ntok, nidx = self._beam_outputs(cand_out, B, k, R)
        nscr = int(self.lib.kmb_beam_step_processed_scratch(R, int(t), n_bad))
        scr = self.__dict__.get("_beam_process_scratch")
        if scr is None or scr.numel() < nscr:
            scr = self._beam_process_scratch = torch.empty(nscr, dtype=torch.float32, device=self.device)
        head = (ptr(add), int(force_token), int(ban_token), int(k), ptr(cand), int(eos_token), ptr(nscore), ptr(ntok), ptr(nidx),
                ptr(scr), scr.numel(), ptr(ids_in), ptr(ids_out), ids_in.stride(0), int(t), float(repetition_penalty),
                int(no_repeat_ngram_size), ptr(btok) if n_bad > 0 else None, ptr(boff) if n_bad > 0 else None, n_bad)
        return self._beam_call(
            logits, outs, reorder_step,
            lambda: self.lib.kmb_gen_beam_step_processed(self.h, ptr(logits), logits.stride(0), int(num_beams), *head,
                                                         int(reorder_step), _stream()),
            lambda: self.lib.kmb_beam_step_processed(ptr(logits), logits.stride(0), V, B, int(num_beams), *head, _stream()),
            forced=force_token >= 0)

    def beam_sample_step(self, logits, num_beams, noise, add=None, temperature=1.0, top_k=0, top_p=1.0, ban_token=-1, eos_token=-1,
                         cand_out=None, reorder_step=-1):
        """One beam-sampling step (kmb_beam_sample_step): per row log_softmax, EOS ban, + add (the beam scores), / temperature,
        top-k / top-p; per batch item k = 2 * num_beams draws without replacement on `noise` (fp32 [B, >= num_beams * V] Exp(1)
        draws), sorted by score, and the next beams (a per-row launch and a per-item merge).  Returns (cand int32 [B, k, 2], next_scores fp32 [R],
        next_tokens int64 [R], next_beam_idx int32 [R]) like beam_step.  reorder_step >= 0: the call also reorders the
        generation caches by next_beam_idx (in the same launch when `logits` are gen_step's, unedited)."""
        R, V = logits.shape[0], int(self.config.vocab_size)
        B, k = R // num_beams, 2 * num_beams
        for x in (logits, noise, add):
            assert x is None or (x.device == self.device and x.dtype == torch.float32 and x.stride(-1) == 1), "beam_sample_step: bad tensor"
        assert R == B * num_beams and noise.shape[0] == B and (add is None or add.numel() == R)
        outs = cand, nscore, ntok, nidx = self._beam_outputs(cand_out, B, k, R)
        nscr = int(self.lib.kmb_beam_sample_scratch(R))
        scr = self.__dict__.get("_beam_sample_scratch")
        if scr is None or scr.numel() < nscr:
            scr = self._beam_sample_scratch = torch.empty(nscr, dtype=torch.float32, device=self.device)
        args = (float(temperature), int(top_k), float(top_p), int(ban_token), ptr(noise), noise.stride(0), int(k), ptr(cand),
                int(eos_token), ptr(nscore), ptr(ntok), ptr(nidx), ptr(scr), scr.numel())
        return self._beam_call(
            logits, outs, reorder_step,
            lambda: self.lib.kmb_gen_beam_sample_step(self.h, ptr(logits), logits.stride(0), int(num_beams), ptr(add), *args,
                                                      int(reorder_step), _stream()),
            lambda: self.lib.kmb_beam_sample_step(ptr(logits), logits.stride(0), V, B, int(num_beams), ptr(add), *args, _stream()))

    def sample_step(self, logits, noise, temperature=1.0, top_k=0, top_p=1.0, ban_token=-1, unfinished=None, pad_token=0,
                    eos_token=-1, next_tokens=None, ids=None, t=0, flag=None, info_out=None, logprob_sum=None, logprob_out=None,
                    embed_step=-1):
        """One decode step's sampling tail (kmb_sample_step): EOS ban, temperature, top-k, top-p and the exponential-race
        draw on `noise` (fp32 [R, >= V] Exp(1) draws) in one launch.  `logits` may be gen_step's padded view.  Returns
        next_tokens (int64 [R]); unfinished (int64 [R]) and the id buffer ids (int64 [R, ld], column t) are updated in place;
        flag (int32, one element) is OR-ed with 1 while a row is unfinished; info_out (fp32 [R, 2]): kept count, smallest
        kept value.
        logprob_sum (fp32 [R]) gains the chosen token's log-probability under the filtered distribution for the rows unfinished
        on entry, logprob_out (fp32, R elements, may be a strided column view) receives this step's (0 for a finished row):
        the same launch, the same tokens (kmb_sample_scored_step).  embed_step >= 0, when `logits` are gen_step's, unedited
        since (their _version unchanged): the launch also embeds the chosen tokens for that decode step
        (kmb_gen_sample_step), and gen_step(next_tokens, embed_step) then runs without an embedding launch, as after
        greedy_step.  With none of the three given the call is kmb_sample_step itself."""
        R, V = logits.shape[0], int(self.config.vocab_size)
        for x, dt in ((logits, torch.float32), (noise, torch.float32), (unfinished, torch.int64), (ids, torch.int64),
                      (flag, torch.int32), (info_out, torch.float32), (logprob_sum, torch.float32)):
            assert x is None or (x.device == self.device and x.dtype == dt and x.stride(-1) == 1), "sample_step: bad tensor"
        assert noise.shape[0] == R and (unfinished is None or unfinished.numel() == R) and (ids is None or ids.shape[0] == R)
        assert info_out is None or info_out.is_contiguous() and info_out.numel() == 2 * R
        assert logprob_sum is None or (logprob_sum.is_contiguous() and logprob_sum.numel() == R)
        assert logprob_out is None or (logprob_out.device == self.device and logprob_out.dtype == torch.float32
                                       and logprob_out.dim() == 1 and logprob_out.numel() == R
                                       and (R == 1 or logprob_out.stride(0) >= 1)), "sample_step: bad logprob_out"
        if next_tokens is None:
            next_tokens = torch.empty((R,), dtype=torch.int64, device=self.device)
        assert next_tokens.is_contiguous() and next_tokens.numel() == R and next_tokens.dtype == torch.int64
        args = (float(temperature), int(top_k), float(top_p), int(ban_token), ptr(noise), noise.stride(0), ptr(unfinished),
                int(pad_token), int(eos_token), ptr(next_tokens), ptr(ids), int(t), ids.stride(0) if ids is not None else 0,
                ptr(flag), ptr(info_out))
        self._folded = None   # next_tokens may be the buffer an earlier step's pending embedding was recorded for
        with torch.cuda.device(self.device):
            if logprob_sum is None and logprob_out is None and embed_step == -1:
                check(self.lib.kmb_sample_step(ptr(logits), logits.stride(0), V, R, *args, _stream()))
                return next_tokens
            scored = (ptr(logprob_sum), ptr(logprob_out), max(int(logprob_out.stride(0)), 1) if logprob_out is not None else 1)
            if logits is self.__dict__.get("_gen_logits") and logits._version == self._gen_logits_version:
                check(self.lib.kmb_gen_sample_step(self.h, ptr(logits), logits.stride(0), *args, *scored, int(embed_step), _stream()))
                if embed_step >= 0 and self.lib.kmb_gen_embedded_step(self.h) == embed_step:
                    self._folded = (next_tokens, next_tokens._version, int(embed_step))
            else:
                check(self.lib.kmb_sample_scored_step(ptr(logits), logits.stride(0), V, R, *args, *scored, _stream()))
        return next_tokens

    def greedy_step(self, logits, ban_token=-1, unfinished=None, pad_token=0, eos_token=-1, next_tokens=None, ids=None, t=0,
                    flag=None, logprob_sum=None, logprob_out=None, embed_step=-1):
        """One decode step's greedy tail (kmb_greedy_step): EOS ban, argmax (lowest index on ties), the chosen token's
        log-probability and the finished-row bookkeeping in one launch.  `logits` may be gen_step's padded view.  Returns
        next_tokens (int64 [R]); unfinished (int64 [R]) and the id buffer ids (int64 [R, ld], column t) are updated in place;
        flag (int32, one element) is OR-ed with 1 while a row is unfinished; logprob_sum (fp32 [R]) gains the log-probability
        of the rows unfinished on entry, logprob_out (fp32 [R]) receives this step's (0 for a finished row).
        embed_step >= 0, when `logits` are gen_step's, unedited since (their _version unchanged): the launch also embeds the
        chosen tokens for that decode step (kmb_gen_greedy_step), and gen_step(next_tokens, embed_step) then runs without an
        embedding launch, as after beam_step."""
        R, V = logits.shape[0], int(self.config.vocab_size)
        for x, dt in ((logits, torch.float32), (unfinished, torch.int64), (ids, torch.int64), (flag, torch.int32),
                      (logprob_sum, torch.float32), (logprob_out, torch.float32)):
            assert x is None or (x.device == self.device and x.dtype == dt and x.stride(-1) == 1), "greedy_step: bad tensor"
        assert (unfinished is None or unfinished.numel() == R) and (ids is None or ids.shape[0] == R)
        assert all(x is None or (x.is_contiguous() and x.numel() == R) for x in (logprob_sum, logprob_out))
        if next_tokens is None:
            next_tokens = torch.empty((R,), dtype=torch.int64, device=self.device)
        assert next_tokens.is_contiguous() and next_tokens.numel() == R and next_tokens.dtype == torch.int64
        self._folded = None
        args = (int(ban_token), ptr(unfinished), int(pad_token), int(eos_token), ptr(next_tokens), ptr(ids), int(t),
                ids.stride(0) if ids is not None else 0, ptr(flag), ptr(logprob_sum), ptr(logprob_out))
        with torch.cuda.device(self.device):
            if logits is self.__dict__.get("_gen_logits") and logits._version == self._gen_logits_version:
                check(self.lib.kmb_gen_greedy_step(self.h, ptr(logits), logits.stride(0), *args, int(embed_step), _stream()))
                if embed_step >= 0 and self.lib.kmb_gen_embedded_step(self.h) == embed_step:
                    self._folded = (next_tokens, next_tokens._version, int(embed_step))
            else:
                check(self.lib.kmb_greedy_step(ptr(logits), logits.stride(0), V, R, *args, _stream()))
        return next_tokens

    def process_logits(self, logits, ids, t, repetition_penalty=1.0, no_repeat_ngram_size=0, bad_words=None):
        """generate()'s score processors on one decode step's logits, in place, in front of greedy_step / sample_step
        (kmb_logits_process): repetition penalty, no-repeat n-grams and bad words from the rows' tokens ids[:, :t] (int64 [R, ld],
        the id buffer the step tails keep; t = the column about to be written).  bad_words: (tokens int32, offsets int32
        [n_bad + 1]) device tensors, the packed table, or None.  `logits` may be gen_step's padded view: the call then takes its
        decode-loop form (kmb_gen_logits_process).  Only raw pointers are passed -- torch sees no in-place op, the logits'
        _version stays the one gen_step left, and the step tail behind this call keeps its kmb_gen_* form with the folded
        embedding."""
        R, V = logits.shape[0], int(self.config.vocab_size)
        assert logits.device == self.device and logits.dtype == torch.float32 and logits.dim() == 2 and logits.stride(1) == 1, \
            "process_logits: bad logits"
        assert ids.device == self.device and ids.dtype == torch.int64 and ids.dim() == 2 and ids.stride(1) == 1 \
            and ids.shape[0] == R, "process_logits: bad ids"
        btok = boff = None
        n_bad = 0
        if bad_words is not None:
            btok, boff = bad_words
            for x in (btok, boff):
                assert x.device == self.device and x.dtype == torch.int32 and x.is_contiguous(), "process_logits: bad table"
            n_bad = boff.numel() - 1
            assert n_bad >= 0 and (n_bad == 0 or btok.numel() > 0)
        with torch.cuda.device(self.device):
            args = (ptr(ids), ids.stride(0), int(t), float(repetition_penalty), int(no_repeat_ngram_size),
                    ptr(btok) if n_bad > 0 else None, ptr(boff) if n_bad > 0 else None, n_bad, _stream())
            if logits is self.__dict__.get("_gen_logits"):
                check(self.lib.kmb_gen_logits_process(self.h, ptr(logits), logits.stride(0), *args))
            else:
                check(self.lib.kmb_logits_process(ptr(logits), logits.stride(0), V, R, *args))
        return logits

    def _topk_scratch_for(self, R):
        nscr = int(self.lib.kmb_logsoftmax_topk_scratch(R))
        scr = self.__dict__.get("_topk_scratch")
        if scr is None or scr.numel() < nscr:
            scr = self._topk_scratch = torch.empty(nscr, dtype=torch.float32, device=self.device)
        return scr

    def logsoftmax_topk(self, logits, k, add=None, force_token=-1, ban_token=-1):
        R = logits.shape[0]
        val = torch.empty((R, k), dtype=torch.float32, device=self.device)
        idx = torch.empty((R, k), dtype=torch.int32, device=self.device)
        scr = self._topk_scratch_for(R)
        with torch.cuda.device(self.device):
            check(self.lib.kmb_logsoftmax_topk_ws(ptr(logits), logits.stride(0), int(self.config.vocab_size), R,
                                                  ptr(add), int(force_token), int(ban_token), int(k), ptr(val), ptr(idx),
                                                  ptr(scr), scr.numel(), _stream()))
        return val, idx
