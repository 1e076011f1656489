"""ctypes binding of libkmbart_hip.so (include/kmbart.h).  Fails loudly when the library is missing:
there is no CPU fallback for the hot path."""
import ctypes as C
import os

import torch  # noqa: F401  -- must come first: torch bundles its own HIP runtime (libamdhip64.so.7); loading ours
#                              before it would map a second runtime from /opt/rocm and break stream sharing

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("KMB_LIB_PATH") or os.path.join(os.path.dirname(_HERE), "lib", "libkmbart_hip.so")   # KMB_LIB_PATH: a diagnostic build of the same library

c_p = C.c_void_p
i32, i64, u32, f32, f64 = C.c_int32, C.c_int64, C.c_uint32, C.c_float, C.c_double


class KmbConfig(C.Structure):
    _fields_ = [(n, i32) for n in (
        "vocab_size", "d_model", "encoder_layers", "decoder_layers", "encoder_attention_heads",
        "decoder_attention_heads", "encoder_ffn_dim", "decoder_ffn_dim", "max_position_embeddings",
        "extra_pos_embeddings", "image_feature_size", "pad_token_id", "bos_token_id", "eos_token_id",
        "img_feat_id", "cls_token_id", "scale_embedding")] + [
        ("dropout", f32), ("attention_dropout", f32), ("activation_dropout", f32), ("layer_norm_eps", f32),
        ("num_labels", i32), ("num_attributes", i32), ("num_relations", i32)]


class KmbBatch(C.Structure):
    _fields_ = [("B", i32), ("S", i32), ("T", i32),
                ("input_ids", c_p), ("attention_mask", c_p), ("image_features", c_p), ("feat_offsets", c_p),
                ("n_features", i32), ("decoder_input_ids", c_p), ("decoder_attention_mask", c_p), ("labels", c_p)]


class KmbPretrain(C.Structure):
    _fields_ = [("n_mrm", i32), ("mrm_rows", c_p), ("mrm_targets", c_p),
                ("n_attr", i32), ("attr_rows", c_p), ("attr_labels", c_p),
                ("n_rel", i32), ("rel_obj_rows", c_p), ("rel_subj_rows", c_p), ("rel_labels", c_p),
                ("lm_factor", f32), ("mrm_factor", f32), ("attr_factor", f32), ("rel_factor", f32),
                ("losses_out", c_p)]


class KmbForwardOpts(C.Structure):
    _fields_ = [("encoder_states", c_p), ("decoder_states_out", c_p), ("skip_head", i32),
                ("row_weights", c_p), ("loss_reduction", i32)]
    # kmb_forward_opts.targets_per_input: the int32 behind loss_reduction, in what was the struct's tail padding (sizeof is unchanged, a zeroed
    # record means one target per input).  It is a property on that word, not a ctypes field: tests/test_loss_weights_cpu.py pins _fields_ as
    # ending in row_weights, loss_reduction, and tests/test_grouped_targets_cpu.py pins this offset against the library's sizeof.
    _TPI_OFFSET = 36

    @property
    def targets_per_input(self):
        return i32.from_address(C.addressof(self) + self._TPI_OFFSET).value

    @targets_per_input.setter
    def targets_per_input(self, g):
        i32.from_address(C.addressof(self) + self._TPI_OFFSET).value = int(g)


class KmbGemm(C.Structure):
    _fields_ = [("A", c_p), ("B", c_p), ("lda", i32), ("ldb", i32), ("a_kc", i32), ("b_kc", i32),
                ("M", i32), ("N", i32), ("K", i32), ("bias", c_p), ("col_scale", f32), ("col_scale_n", i32),
                ("act", i32), ("preact", c_p), ("ld_preact", i32), ("aux", c_p), ("ld_aux", i32),
                ("drop_thr16", u32), ("drop_seed", u32), ("drop_scale", f32), ("residual", c_p), ("ld_res", i32),
                ("out_bf16", c_p), ("ld_out_bf16", i32), ("out_f32", c_p), ("ld_out_f32", i32), ("beta", f32),
                ("split_k", i32), ("slab", c_p), ("colsum", c_p), ("tile_order", i32),
                ("row_shift", c_p), ("row_sums", c_p), ("row_sums_ld", i32), ("pick_col", c_p), ("pick_out", c_p)]


class KmbAttn(C.Structure):
    _fields_ = [("Q", c_p), ("K", c_p), ("V", c_p), ("ldq", i32), ("ldk", i32), ("ldv", i32),
                ("B", i32), ("H", i32), ("Tq", i32), ("Tk", i32), ("key_mask", c_p), ("causal", i32),
                ("O", c_p), ("ldo", i32), ("lse", c_p), ("dO", c_p), ("lddo", i32),
                ("dQ", c_p), ("dK", c_p), ("dV", c_p), ("lddq", i32), ("lddk", i32), ("lddv", i32),
                ("dq_scale", f32), ("dq_colsum", c_p), ("dk_colsum", c_p), ("dv_colsum", c_p), ("ld_colsum", i32),
                ("drop_thr16", u32), ("drop_seed", u32), ("drop_scale", f32)]


class KmbAttnDecode(C.Structure):
    _fields_ = [("Q", c_p), ("ldq", i32), ("Kc", c_p), ("Vc", c_p), ("Tmax", i32), ("ldc", i32), ("kv_row", c_p),
                ("key_mask", c_p), ("mask_ld", i32), ("mask_row", c_p), ("R", i32), ("H", i32), ("Tk", i32),
                ("O", c_p), ("ldo", i32), ("new_k", c_p), ("new_v", c_p), ("ld_new", i32), ("Kw", c_p), ("Vw", c_p), ("hist", c_p)]


class KmbDecodeBlock(C.Structure):
    _fields_ = [("kind", i32), ("in_", c_p), ("ld_in", i32), ("gamma", c_p), ("beta", c_p), ("eps", f32), ("ln_out", c_p),
                ("W", c_p), ("bias", c_p), ("R", i32), ("K", i32), ("N", i32), ("act", i32), ("residual", c_p),
                ("ld_res", i32), ("out", c_p), ("ld_out", i32), ("H", i32), ("q_scale", f32), ("Kc", c_p), ("Vc", c_p),
                ("Tmax", i32), ("ldc", i32), ("Tk", i32), ("kv_row", c_p), ("key_mask", c_p), ("mask_ld", i32), ("hist", c_p), ("kv_group", i32),
                ("w_format", i32), ("w_exp", c_p)]   # appended: a zeroed record is a bf16 block


# KmbDecodeBlock.w_format / kmb_gen_set_weight_format (include/kmbart.h KMB_WFMT_*)
WEIGHT_FORMATS = {"bf16": 0, "fp8_e4m3": 1}


# kmb_debug_decode_route: the kernel a decode block runs (include/kmbart.h KMB_DECODE_ROUTE_*)
DECODE_ROUTES = ("proj_wide", "proj2", "proj4", "proj6", "attn_self", "attn_cross", "attn_cross_kvlds")
# kmb_debug_attn_route: the kernel an attention forward / backward runs (include/kmbart.h KMB_ATTN_ROUTE_*)
ATTN_ROUTES = ("general", "small", "small_pack", "qstream")


class KmbDrop(C.Structure):
    _fields_ = [("thr16", u32), ("seed", u32), ("scale", f32)]


class KmbAdamW(C.Structure):
    _fields_ = [("lr", f64), ("beta1", f64), ("beta2", f64), ("eps", f64), ("weight_decay", f64),
                ("step", i32), ("correct_bias", i32), ("grad_scale", f32)]


class KmbStepState(C.Structure):
    """The device record of a clipped / guarded optimizer step (include/kmbart.h)."""
    _fields_ = [("norm", f32), ("coef", f32), ("step_size", f32), ("applied", i32), ("steps", i32), ("skipped", i32)]


class KmbAllreduceOpts(C.Structure):
    _fields_ = [("algo", i32), ("after_compute", i32), ("max_piece_elems", i64), ("adamw", C.POINTER(KmbAdamW))]


class KmbCommPiece(C.Structure):
    _fields_ = [("bucket", i32), ("repad_piece", i32), ("repad_shard", i32), ("reserved", i32),
                ("offset", i64), ("count", i64), ("shard", i64), ("mine", i64)]


# name -> (restype, argtypes); must list every function include/kmbart.h declares
PROTOTYPES = {
    "kmb_last_error": (C.c_char_p, []),
    "kmb_version": (C.c_int, []),
    "kmb_create": (C.c_int, [C.POINTER(KmbConfig), C.POINTER(c_p)]),
    "kmb_destroy": (None, [c_p]),
    "kmb_param_count": (C.c_int, [c_p]),
    "kmb_param_info": (C.c_int, [c_p, C.c_int, C.POINTER(C.c_char_p), C.POINTER(i64), C.POINTER(i32), C.POINTER(i32)]),
    "kmb_arena_elems": (i64, [c_p]),
    "kmb_bf16_arena_elems": (i64, [c_p]),
    "kmb_bind_arenas": (C.c_int, [c_p, c_p, c_p, c_p, c_p, c_p, c_p]),
    "kmb_workspace_bytes": (i64, [c_p, C.c_int, C.c_int, C.c_int, C.c_int]),
    "kmb_workspace_bytes_grouped": (i64, [c_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int]),
    "kmb_bind_workspace": (C.c_int, [c_p, c_p, i64]),
    "kmb_sync_params": (C.c_int, [c_p, c_p]),
    "kmb_set_seed": (C.c_int, [c_p, C.c_uint64]),
    "kmb_set_attention_dropout": (C.c_int, [c_p, f32]),
    "kmb_attention_dropout_site": (C.c_int, [c_p, C.c_int, C.c_int, C.POINTER(u32), C.POINTER(u32)]),
    "kmb_set_activation_dropout": (C.c_int, [c_p, f32]),
    "kmb_activation_dropout_site": (C.c_int, [c_p, C.c_int, C.c_int, C.POINTER(u32), C.POINTER(u32)]),
    "kmb_set_classif_dropout": (C.c_int, [c_p, f32]),
    "kmb_classif_dropout_site": (C.c_int, [c_p, C.c_int, C.c_int, C.POINTER(u32), C.POINTER(u32)]),
    "kmb_set_label_smoothing": (C.c_int, [c_p, f32]),
    "kmb_last_head_form": (C.c_int, [c_p]),
    "kmb_abi_sizeof_attn":(C.c_int, []),
    "kmb_abi_sizeof_forward_opts": (C.c_int, []),
    "kmb_bucket_count": (C.c_int, [c_p]),
    "kmb_bucket_range": (C.c_int, [c_p, C.c_int, C.POINTER(i64), C.POINTER(i64)]),
    "kmb_stream_wait_bucket": (C.c_int, [c_p, C.c_int, c_p]),
    "kmb_logits_ld": (C.c_int, [c_p]),
    "kmb_forward": (C.c_int, [c_p, C.POINTER(KmbBatch), C.c_int, C.c_int, c_p, c_p, c_p, c_p]),
    "kmb_forward_ex": (C.c_int, [c_p, C.POINTER(KmbBatch), C.POINTER(KmbForwardOpts), C.c_int, C.c_int, c_p, c_p, c_p, c_p]),
    "kmb_score": (C.c_int, [c_p, C.POINTER(KmbBatch), c_p, c_p, c_p, C.POINTER(i32), c_p]),
    "kmb_last_logits": (C.c_int, [c_p, c_p, c_p]),
    "kmb_hidden_state": (C.c_int, [c_p, C.c_int, C.c_int, c_p, c_p]),
    "kmb_attention_probs": (C.c_int, [c_p, C.c_int, C.c_int, c_p, c_p]),
    "kmb_set_precision": (C.c_int, [c_p, C.c_int]),
    "kmb_act_bytes": (C.c_int, [c_p]),
    "kmb_reserve_head_rows": (C.c_int, [c_p, C.c_int]),
    "kmb_forward_pretrain": (C.c_int, [c_p, C.POINTER(KmbBatch), C.POINTER(KmbPretrain), C.c_int, C.c_int, c_p, c_p, c_p]),
    "kmb_forward_pretrain_ex": (C.c_int, [c_p, C.POINTER(KmbBatch), C.POINTER(KmbPretrain), C.POINTER(KmbForwardOpts), C.c_int, C.c_int,
                                          c_p, c_p, c_p]),
    "kmb_backward": (C.c_int, [c_p, f32, c_p]),
    "kmb_backward_dev": (C.c_int, [c_p, c_p, c_p]),
    "kmb_adamw_step": (C.c_int, [c_p, C.POINTER(KmbAdamW), i64, i64, c_p]),
    "kmb_step_state_bytes": (i64, [c_p]),
    "kmb_bind_step_state": (C.c_int, [c_p, c_p, i64]),
    "kmb_grad_sumsq": (C.c_int, [c_p, i64, i64, f32, i32, c_p]),
    "kmb_clip_finish": (C.c_int, [c_p, C.POINTER(KmbAdamW), f32, i32, i32, c_p]),
    "kmb_adamw_step_dev": (C.c_int, [c_p, C.POINTER(KmbAdamW), i64, i64, c_p]),
    "kmb_step_state_read": (C.c_int, [c_p, c_p, c_p]),
    "kmb_step_state_set_steps": (C.c_int, [c_p, i32, c_p]),
    "kmb_bind_grad_stage": (C.c_int, [c_p, c_p, i64]),
    "kmb_set_grad_accumulation": (C.c_int, [c_p, C.c_int]),
    "kmb_zero_grad": (C.c_int, [c_p]),
    "kmb_read_status": (C.c_int, [c_p, C.POINTER(i32), c_p]),
    "kmb_read_status_async": (C.c_int, [c_p, c_p, c_p]),
    "kmb_gen_begin": (C.c_int, [c_p, C.POINTER(KmbBatch), C.c_int, C.c_int, c_p]),
    "kmb_gen_encoder_states": (C.c_int, [c_p, c_p, c_p]),
    "kmb_gen_step": (C.c_int, [c_p, c_p, C.c_int, c_p, c_p]),
    "kmb_gen_reorder": (C.c_int, [c_p, c_p, C.c_int, c_p]),
    "kmb_gen_last_hidden": (C.c_int, [c_p, c_p, c_p]),
    "kmb_gen_embedded_step": (C.c_int, [c_p]),
    "kmb_gen_stats_blocks": (C.c_int, [c_p, c_p]),
    "kmb_beam_merge": (C.c_int, [c_p, c_p, C.c_int, C.c_int, C.c_int, C.c_int, c_p, c_p]),
    "kmb_beam_merge_select": (C.c_int, [c_p, c_p, C.c_int, C.c_int, C.c_int, C.c_int, c_p, C.c_int, c_p, c_p, c_p, c_p]),
    "kmb_beam_step": (C.c_int, [c_p, C.c_int, C.c_int, C.c_int, C.c_int, c_p, C.c_int, C.c_int, C.c_int, c_p, C.c_int, c_p, c_p, c_p,
                                c_p, C.c_int64, c_p]),
    "kmb_gen_beam_step": (C.c_int, [c_p, c_p, C.c_int, C.c_int, c_p, C.c_int, C.c_int, C.c_int, c_p, C.c_int, c_p, c_p, c_p,
                                    c_p, C.c_int64, C.c_int, c_p]),
    "kmb_beam_step_stats": (C.c_int, [c_p, C.c_int, C.c_int, C.c_int, C.c_int, c_p, C.c_int, C.c_int, C.c_int, c_p, C.c_int, c_p, c_p,
                                      c_p, c_p, C.c_int, c_p]),
    "kmb_logsoftmax_topk": (C.c_int, [c_p, C.c_int, C.c_int, C.c_int, c_p, C.c_int, C.c_int, C.c_int, c_p, c_p, c_p]),
    "kmb_logsoftmax_topk_scratch": (C.c_int64, [C.c_int]),
    "kmb_logsoftmax_topk_ws": (C.c_int, [c_p, C.c_int, C.c_int, C.c_int, c_p, C.c_int, C.c_int, C.c_int, c_p, c_p, c_p,
                                         C.c_int64, c_p]),
    "kmb_sample_step": (C.c_int, [c_p, C.c_int, C.c_int, C.c_int, f32, C.c_int, f32, C.c_int, c_p, C.c_int, c_p, i64, i64, c_p,
                                  c_p, C.c_int, C.c_int, c_p, c_p, c_p]),
    "kmb_sample_scored_step": (C.c_int, [c_p, C.c_int, C.c_int, C.c_int, f32, C.c_int, f32, C.c_int, c_p, C.c_int, c_p, i64, i64, c_p,
                                         c_p, C.c_int, C.c_int, c_p, c_p, c_p, c_p, C.c_int, c_p]),
    "kmb_gen_sample_step": (C.c_int, [c_p, c_p, C.c_int, f32, C.c_int, f32, C.c_int, c_p, C.c_int, c_p, i64, i64, c_p,
                                      c_p, C.c_int, C.c_int, c_p, c_p, c_p, c_p, C.c_int, C.c_int, c_p]),
    "kmb_greedy_step": (C.c_int, [c_p, C.c_int, C.c_int, C.c_int, C.c_int, c_p, i64, i64, c_p, c_p, C.c_int, C.c_int, c_p, c_p, c_p, c_p]),
    "kmb_gen_greedy_step": (C.c_int, [c_p, c_p, C.c_int, C.c_int, c_p, i64, i64, c_p, c_p, C.c_int, C.c_int, c_p, c_p, c_p, C.c_int,
                                      c_p]),
    "kmb_logits_process": (C.c_int, [c_p, C.c_int, C.c_int, C.c_int, c_p, C.c_int, C.c_int, f32, C.c_int, c_p, c_p, C.c_int, c_p]),
    "kmb_gen_logits_process": (C.c_int, [c_p, c_p, C.c_int, c_p, C.c_int, C.c_int, f32, C.c_int, c_p, c_p, C.c_int, c_p]),
    "kmb_cider_reward": (C.c_int, [c_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, c_p, C.c_int, c_p, c_p, c_p, f32, c_p, C.c_int,
                                   c_p, c_p, c_p, c_p, c_p, i64, C.c_int, f32, c_p, c_p]),
    "kmb_beam_step_processed_scratch": (C.c_int64, [C.c_int, C.c_int, C.c_int]),
    "kmb_beam_step_processed": (C.c_int, [c_p, C.c_int, C.c_int, C.c_int, C.c_int, c_p, C.c_int, C.c_int, C.c_int, c_p, C.c_int, c_p, c_p,
                                          c_p, c_p, C.c_int64, c_p, c_p, C.c_int, C.c_int, f32, C.c_int, c_p, c_p, C.c_int, c_p]),
    "kmb_gen_beam_step_processed": (C.c_int, [c_p, c_p, C.c_int, C.c_int, c_p, C.c_int, C.c_int, C.c_int, c_p, C.c_int, c_p, c_p, c_p,
                                              c_p, C.c_int64, c_p, c_p, C.c_int, C.c_int, f32, C.c_int, c_p, c_p, C.c_int, C.c_int,
                                              c_p]),
    "kmb_beam_sample_step": (C.c_int, [c_p, C.c_int, C.c_int, C.c_int, C.c_int, c_p, f32, C.c_int, f32, C.c_int, c_p, C.c_int,
                                       C.c_int, c_p, C.c_int, c_p, c_p, c_p, c_p, C.c_int64, c_p]),
    "kmb_beam_sample_scratch": (C.c_int64, [C.c_int]),
    "kmb_gen_beam_sample_step": (C.c_int, [c_p, c_p, C.c_int, C.c_int, c_p, f32, C.c_int, f32, C.c_int, c_p, C.c_int, C.c_int, c_p,
                                           C.c_int, c_p, c_p, c_p, c_p, C.c_int64, C.c_int, c_p]),
    "kmb_gen_workspace_bytes": (i64, [c_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int]),
    "kmb_gen_set_weight_format": (C.c_int, [c_p, C.c_int]),
    "kmb_gemm_shared_device": (C.c_int, [C.c_int]),
    "kmb_debug_gemm_route": (C.c_int, [C.POINTER(KmbGemm), C.c_int, c_p, C.c_int32]),
    "kmb_debug_decode_route": (C.c_int, [C.POINTER(KmbDecodeBlock)]),
    "kmb_debug_attn_route": (C.c_int, [C.POINTER(KmbAttn), C.c_int]),
    "kmb_comm_unique_id": (C.c_int, [c_p]),
    "kmb_comm_init": (C.c_int, [c_p, C.c_int, C.c_int, c_p]),
    "kmb_comm_destroy": (C.c_int, [c_p]),
    "kmb_encoder_states_grad": (C.c_int, [c_p, c_p, c_p]),
    "kmb_comm_info": (C.c_int, [c_p, C.POINTER(i32), C.POINTER(i32)]),
    "kmb_comm_broadcast_params": (C.c_int, [c_p, C.c_int, c_p]),
    "kmb_allreduce_grads": (C.c_int, [c_p, C.POINTER(KmbAllreduceOpts), c_p]),
    "kmb_comm_wait": (C.c_int, [c_p, c_p]),
    "kmb_comm_gather_moments": (C.c_int, [c_p, c_p]),
    "kmb_comm_pieces": (i64, [c_p, i64]),
    "kmb_comm_plan": (C.c_int, [c_p, C.c_int, C.c_int, i64, i64, C.POINTER(KmbCommPiece)]),
    "kmb_comm_moments_sharded": (C.c_int, [c_p]),
    "kmb_debug_trace": (C.c_int, [C.c_int]),
    "kmb_debug_trace_dump": (C.c_int, [C.c_char_p]),
    "kmb_set_side_stream": (C.c_int, [c_p, C.c_int]),
    "kmb_profile_gemm": (C.c_int, [C.c_int]),
    "kmb_profile_read": (C.c_int, [C.c_int, C.POINTER(i64), C.POINTER(f64), C.POINTER(f64)]),
    "kmb_profile_dump": (C.c_int, [C.c_char_p]),
    "kmb_clock_stamp": (C.c_int, [c_p, c_p]),
    "kmb_pack_features": (C.c_int, [c_p, c_p, C.c_int32, C.c_int32, c_p, c_p]),
    "kmb_op_gemm": (C.c_int, [C.POINTER(KmbGemm), c_p]),
    "kmb_op_gemm_allrows": (C.c_int, [C.POINTER(KmbGemm), c_p]),
    "kmb_op_gemm_allrows_stats_floats": (C.c_int64, [C.c_int]),
    "kmb_op_gemm_allrows_stats": (C.c_int, [C.POINTER(KmbGemm), c_p, c_p]),
    "kmb_op_gemm_score_stats_floats": (C.c_int64, [C.c_int, C.c_int]),
    "kmb_op_gemm_score": (C.c_int, [C.POINTER(KmbGemm), c_p, c_p]),
    "kmb_op_score_rows_finish": (C.c_int, [c_p, C.c_int, c_p, c_p, C.c_int, C.c_int, C.c_int, c_p, c_p, c_p, c_p]),
    "kmb_op_gemm_group": (C.c_int, [C.POINTER(KmbGemm), C.c_int32, c_p]),
    "kmb_op_attn_fwd": (C.c_int, [C.POINTER(KmbAttn), c_p]),
    "kmb_op_attn_bwd": (C.c_int, [C.POINTER(KmbAttn), c_p]),
    "kmb_op_attn_decode": (C.c_int, [C.POINTER(KmbAttnDecode), c_p]),
    "kmb_op_decode_block": (C.c_int, [C.POINTER(KmbDecodeBlock), c_p]),
    "kmb_op_decode_pack": (C.c_int, [c_p, C.c_int, C.c_int, C.c_int, c_p, c_p]),
    "kmb_op_decode_pack_fp8": (C.c_int, [c_p, C.c_int, C.c_int, C.c_int, c_p, c_p, c_p]),
    "kmb_abi_sizeof_decode_block": (C.c_int, []),
    "kmb_op_ln_fwd": (C.c_int, [c_p, c_p, c_p, c_p, c_p, c_p, C.c_int, C.c_int, f32, c_p]),
    "kmb_op_ln_bwd_scratch": (i64, [C.c_int, C.c_int]),
    "kmb_op_ln_bwd": (C.c_int, [c_p, c_p, c_p, c_p, c_p, c_p, c_p, C.POINTER(KmbDrop), C.POINTER(KmbDrop), c_p, c_p,
                                c_p, C.c_int, C.c_int, c_p]),
    "kmb_op_ln_bwd_sub": (C.c_int, [c_p, c_p, c_p, c_p, c_p, c_p, c_p, C.POINTER(KmbDrop), C.POINTER(KmbDrop), c_p, c_p,
                                    c_p, c_p, C.c_int, C.c_int, c_p]),
    "kmb_op_ln_fwd_slabs": (C.c_int, [c_p, C.c_int, i64, c_p, c_p, C.c_int, c_p, c_p, c_p, C.c_int, C.c_int, f32, c_p]),
    "kmb_op_reduce_slabs": (C.c_int, [c_p, C.c_int, i64, c_p, i64, f32, c_p]),
    "kmb_op_reduce_slabs_bf16": (C.c_int, [c_p, C.c_int, i64, c_p, i64, c_p]),
    "kmb_op_reduce_slabs_epi": (C.c_int, [c_p, C.c_int, i64, c_p, f32, C.c_int, C.POINTER(KmbDrop), c_p, C.c_int, c_p, C.c_int,
                                          C.c_int, C.c_int, c_p]),
    "kmb_op_colsum_scratch": (i64, [C.c_int, C.c_int]),
    "kmb_op_colsum": (C.c_int, [c_p, C.c_int, C.c_int, C.c_int, c_p, c_p, c_p]),
    "kmb_op_img_rowmap": (C.c_int, [c_p, c_p, C.c_int, C.c_int, i64, i64, c_p, c_p, c_p]),
    "kmb_op_cast_pad": (C.c_int, [c_p, C.c_int, C.c_int, c_p, C.c_int, c_p]),
    "kmb_op_embed_ln_fwd": (C.c_int, [c_p, c_p, c_p, c_p, c_p, C.c_int, C.c_int, f32, c_p, c_p, c_p, c_p, c_p, c_p,
                                      C.c_int, C.c_int, f32, C.POINTER(KmbDrop), c_p]),
    "kmb_op_embed_bwd": (C.c_int, [c_p, c_p, c_p, f32, c_p, c_p, i64, C.c_int, C.c_int, c_p]),
    "kmb_op_pos_bwd": (C.c_int, [c_p, C.c_int, C.c_int, C.c_int, c_p, C.c_int, C.c_int, c_p]),
    "kmb_op_ce": (C.c_int, [c_p, C.c_int, C.c_int, c_p, C.c_int, f32, c_p, c_p, c_p, c_p, c_p]),
    "kmb_op_ce_bf16": (C.c_int, [c_p, C.c_int, C.c_int, c_p, C.c_int, f32, c_p, c_p, c_p, c_p, c_p, c_p]),
    "kmb_op_count_valid": (C.c_int, [c_p, C.c_int, C.c_int, c_p, c_p, c_p]),
    "kmb_op_loss_finish": (C.c_int, [c_p, C.c_int, c_p, c_p, c_p]),
    "kmb_op_ce_label_logit": (C.c_int, [c_p, C.c_int, c_p, C.c_int, c_p, c_p, C.c_int, C.c_int, C.c_int, C.c_int, c_p, c_p, c_p]),
    "kmb_op_ce_rows_finish": (C.c_int, [c_p, C.c_int, C.c_int, c_p, c_p, c_p, f32, C.c_int, C.c_int, C.c_int, c_p, C.c_int, c_p, c_p,
                                        c_p, c_p, c_p, C.c_int, c_p]),
    "kmb_op_ce_dgrad_finish": (C.c_int, [c_p, C.c_int, i64, c_p, c_p, C.c_int, C.c_int, c_p]),
    "kmb_op_ce_smooth": (C.c_int, [c_p, C.c_int, C.c_int, c_p, C.c_int, f32, f32, c_p, c_p, c_p, c_p, c_p]),
    "kmb_op_ce_bf16_smooth": (C.c_int, [c_p, C.c_int, C.c_int, c_p, C.c_int, f32, f32, c_p, c_p, c_p, c_p, c_p, c_p]),
    "kmb_op_ce_vocab_sum_scratch": (i64, [C.c_int, C.c_int]),
    "kmb_op_ce_vocab_sum": (C.c_int, [c_p, C.c_int, c_p, C.c_int, C.c_int, c_p, c_p, c_p]),
    "kmb_op_ce_rows_finish_smooth_scratch": (i64, [C.c_int, C.c_int]),
    "kmb_op_ce_rows_finish_smooth": (C.c_int, [c_p, C.c_int, C.c_int, c_p, c_p, c_p, c_p, f32, f32, C.c_int, C.c_int, C.c_int, c_p, C.c_int,
                                               c_p, c_p, c_p, c_p, c_p, c_p, c_p, C.c_int, c_p, c_p, c_p]),
    "kmb_op_ce_dgrad_finish_smooth": (C.c_int, [c_p, C.c_int, i64, c_p, c_p, c_p, c_p, C.c_int, C.c_int, c_p]),
    "kmb_op_ce_weighted": (C.c_int, [c_p, C.c_int, C.c_int, c_p, C.c_int, f32, f32, c_p, C.c_int, c_p, c_p, c_p, c_p, c_p]),
    "kmb_op_ce_bf16_weighted": (C.c_int, [c_p, C.c_int, C.c_int, c_p, C.c_int, f32, f32, c_p, C.c_int, c_p, c_p, c_p, c_p, c_p, c_p]),
    "kmb_op_ce_rows_finish_weighted": (C.c_int, [c_p, C.c_int, C.c_int, c_p, c_p, c_p, c_p, f32, f32, c_p, C.c_int, C.c_int, C.c_int, C.c_int,
                                                 c_p, C.c_int, c_p, c_p, c_p, c_p, c_p, c_p, c_p, C.c_int, c_p, c_p, c_p]),
    "kmb_op_reduce_slabs_rowvec": (C.c_int, [c_p, C.c_int, i64, c_p, C.c_int, C.c_int, f32, c_p, c_p]),
    "kmb_op_kl_div":(C.c_int, [c_p, C.c_int, C.c_int, c_p, C.c_int, C.c_int, f32, c_p, c_p, C.c_int, c_p]),
    "kmb_op_gather_rows_bf16": (C.c_int, [c_p, C.c_int, c_p, c_p, C.c_int, C.c_int, C.c_int, c_p]),
    "kmb_op_gather_rows_drop_bf16": (C.c_int, [c_p, C.c_int, c_p, c_p, c_p, C.c_int, C.c_int, C.c_int, C.POINTER(KmbDrop), c_p]),
    "kmb_op_scatter_add_rows": (C.c_int, [c_p, C.c_int, c_p, c_p, C.c_int, C.c_int, c_p]),
    "kmb_op_add_f32_into_bf16": (C.c_int, [c_p, c_p, i64, c_p]),
    "kmb_op_mean_rows": (C.c_int, [c_p, C.c_int, f32, f32, c_p, c_p]),
    "kmb_op_adamw": (C.c_int, [c_p, c_p, c_p, c_p, c_p, i64, C.POINTER(KmbAdamW), c_p]),
    "kmb_op_grad_sumsq": (C.c_int, [c_p, i64, f32, c_p, i32, c_p]),
    "kmb_op_grad_sumsq_slots": (C.c_int, [i64]),
    "kmb_op_grad_fold": (C.c_int, [c_p, c_p, i64, C.c_int, c_p]),
    "kmb_op_clip_finish": (C.c_int, [c_p, i32, f32, i32, C.POINTER(KmbAdamW), c_p, c_p]),
    "kmb_op_adamw_dev": (C.c_int, [c_p, c_p, c_p, c_p, c_p, i64, C.POINTER(KmbAdamW), c_p, c_p]),
    "kmb_op_cast_bf16": (C.c_int, [c_p, c_p, i64, c_p]),
    "kmb_op_dropout_mask": (C.c_int, [u32, f32, C.c_int, C.c_int, c_p, c_p]),
}

_lib = None


class KmbError(RuntimeError):
    pass


def load():
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise KmbError(
            "libkmbart_hip.so is missing (%s). Build it with `python km-bart_amd/build.py`; "
            "the KM-BART hot path has no CPU fallback." % LIB_PATH)
    lib = C.CDLL(LIB_PATH)
    for name, (res, args) in PROTOTYPES.items():
        fn = getattr(lib, name)  # AttributeError if the library does not export a declared symbol
        fn.restype = res
        fn.argtypes = args
    _lib = lib
    return lib


def check(rc):
    if rc != 0:
        raise KmbError(load().kmb_last_error().decode("utf-8", "replace"))


def ptr(t):
    """Device (or host) address of a torch tensor, or NULL."""
    return None if t is None else C.c_void_p(t.data_ptr())
